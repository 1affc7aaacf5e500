"""GPU: csrc/importance.hip through bindings/_importance.py and through models/importance.py -- the sampler against the chain's
functional helper on the same uniforms, the update against the chain (where that is defined) and against the restatement of
tests/importance_ref.py (everywhere), construct_cdf against the restatement bit for bit and against float64 within a derived bound."""
import math
import os
import types

import numpy as np
import pytest
import torch

import importance_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = [(3, 5, 7), (2, 3, 130), (4, 65, 9), (1, 4, 64)]


@pytest.fixture(scope="module")
def I(hiplib):
    from nr3d_lib_amd.models import importance
    saved = importance.FUSED_IMPORTANCE, importance.FUSED_CALLS, importance.CHECK_VAL
    importance.FUSED_IMPORTANCE, importance.FUSED_CALLS = True, frozenset({"sample", "update", "construct_cdf"})
    yield importance
    importance.FUSED_IMPORTANCE, importance.FUSED_CALLS, importance.CHECK_VAL = saved


@pytest.fixture(scope="module")
def B(hiplib):
    from nr3d_lib_amd.bindings import _importance
    return _importance


def seeded_map(shape, seed, zeros=False):
    g = torch.Generator().manual_seed(seed)
    e = torch.empty(shape).uniform_(0.2, 1, generator=g)
    if zeros:                                           # cells without mass: with min_pdf = 0 the CDFs get runs of equal values
        e[torch.rand(shape, generator=g) < 0.3] = 0
    return e


_cdfs = {}


def cdfs_of(B, dev, shape, ties):
    """(cdf_x_cond_y, cdf_y, cdf_img) on the GPU, computed once per case and left unchanged"""
    key = (shape, ties)
    if key not in _cdfs:
        e = seeded_map(shape, 11, zeros=ties).to(dev)
        _cdfs[key] = B.construct_cdf(e, 0.0 if ties else 0.01)
    return _cdfs[key]


def uniforms_for(cx, cy, ci, n_random=4096):
    """u float32 [3, n] and the frames that go with it: first, per (frame f, row h), uniforms that ARE CDF elements -- u_img = cdf_img[f],
    u_y = cdf_y[f, h], u_x = cdf_x_cond_y[f, h, w] for every w (ties take the first index) -- then values below the first elements,
    1e-6 and 1 - 1e-6 on every level, then random values"""
    N, H, W = cx.shape
    dev = cx.device
    f = torch.arange(N, device=dev).repeat_interleave(H * W)
    h = torch.arange(H, device=dev).repeat_interleave(W).repeat(N)
    w = torch.arange(W, device=dev).repeat(N * H)
    exact = torch.stack([ci[f], cx[f, h, w], cy[f, h]])
    lo = torch.stack([ci[0] / 2, cx[0, 0, 0] / 2, cy[0, 0] / 2]).unsqueeze(1)
    ends = torch.tensor([[1e-6, 1 - 1e-6, 1e-6, 1 - 1e-6], [1e-6, 1e-6, 1 - 1e-6, 1 - 1e-6], [1 - 1e-6, 1e-6, 1 - 1e-6, 1e-6]], device=dev)
    rnd = torch.rand(3, n_random, generator=torch.Generator().manual_seed(5)).to(dev)
    u = torch.cat([exact, lo, ends, rnd], dim=1).float().clamp_(1e-6, 1 - 1e-6).contiguous()
    frames = torch.cat([f, torch.randint(N, [u.shape[1] - f.shape[0]], generator=torch.Generator().manual_seed(6)).to(dev)])
    return u, frames


# ---- sampling --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_equals_the_chain_helper(I, B, dev, shape, ties):
    cx, cy, ci = cdfs_of(B, dev, shape, ties)
    u, frames = uniforms_for(cx, cy, ci)
    n = u.shape[1]
    # the chain's helper runs on CPU copies: the division by the resolution is a true division there, as in the kernel and in the
    # reference's recorded CPU values; on the GPU torch divides by a Python scalar through a multiplication with its reciprocal
    cx_c, cy_c, ci_c, u_c = cx.cpu(), cy.cpu(), ci.cpu(), u.cpu()
    for frame_ind in (None, shape[0] - 1, frames):
        u_img = u[0] if frame_ind is None else None
        i_f, xy_f = I.errmap_sample_from_uniform(ci, cy, cx, frame_ind, u_img, u[1], u[2], fused=True)
        i_c, xy_c = I.errmap_sample_from_uniform(ci_c, cy_c, cx_c, frame_ind.cpu() if isinstance(frame_ind, torch.Tensor) else frame_ind,
                                                 None if u_img is None else u_c[0], u_c[1], u_c[2])
        assert xy_f.shape == (n, 2) and xy_f.dtype == torch.float32
        if frame_ind is None:
            assert i_f.dtype == torch.int64 and torch.equal(i_f.cpu(), i_c)
            if not ties:                                    # u_img = cdf_img[f] exactly: the first index whose element is >= u is f
                n_exact = shape[0] * shape[1] * shape[2]
                assert torch.equal(i_f[:n_exact], frames[:n_exact])
        assert torch.equal(xy_f.cpu(), xy_c), (shape, ties, type(frame_ind).__name__, (xy_f.cpu() != xy_c).sum().item())
        # the chain on the GPU: the same bins, positions one rounding of the reciprocal apart
        xy_g = I.errmap_sample_from_uniform(ci, cy, cx, frame_ind, u_img, u[1], u[2])[1]
        torch.testing.assert_close(xy_g, xy_f, rtol=4 * 2.0 ** -24, atol=0)
    # ... and the restatement on the special values and a few random ones (the chain and the kernel agree above; this pins both)
    k = min(n - 4096 + 64, 600)
    sel = torch.cat([torch.arange(k // 2), torch.arange(n - 4096 - 5 - k // 2, n - 4096 + 64)]).to(dev)
    us = u[:, sel].contiguous()
    i_f, xy_f = I.errmap_sample_from_uniform(ci, cy, cx, None, us[0], us[1], us[2], fused=True)
    ri, rxy = ref.sample(ci.cpu().numpy(), cy.cpu().numpy(), cx.cpu().numpy(), None, *us.cpu().numpy())
    assert np.array_equal(i_f.cpu().numpy(), ri) and np.array_equal(xy_f.cpu().numpy(), rxy)
    assert bool((xy_f >= 0).all()) and bool((xy_f <= 1).all())
    # frames only, and frames given as negative indices
    assert torch.equal(I.errmap_sample_from_uniform(ci, cy, cx, None, u[0], None, None, fused=True)[0],
                       torch.searchsorted(ci, u[0], right=False))
    assert torch.equal(I.errmap_sample_from_uniform(None, cy, cx, -1, None, u[1], u[2], fused=True)[1],
                       I.errmap_sample_from_uniform(None, cy, cx, shape[0] - 1, None, u[1], u[2], fused=True)[1])


def test_sample_index_clamp_keeps_reads_inside_the_row(B, dev):
    """rows whose last element is below u: the index is len - 1, nothing behind the row is read into the result or written"""
    guard = 7.0
    buf_y = torch.tensor([0.1, 0.2, 0.3, 0.5] + [guard] * 4, device=dev)
    buf_x = torch.tensor([0.1, 0.2, 0.25] * 4 + [guard] * 4, device=dev)
    buf_i = torch.tensor([0.4] + [guard] * 4, device=dev)
    cy, cx, ci = buf_y[:4].view(1, 4), buf_x[:12].view(1, 4, 3), buf_i[:1]
    u = torch.tensor([[0.9, 0.45], [0.9, 0.6], [0.9, 0.05]], device=dev)
    i, xy = B.sample([(ci, cy, cx)], [0], 0, 1, u[0], u[1], u[2])
    assert i.tolist() == [0, 0]
    ri, rxy = ref.sample(ci.cpu().numpy(), cy.cpu().numpy(), cx.cpu().numpy(), None, *u.cpu().numpy())
    assert np.array_equal(xy.cpu().numpy(), rxy)
    # sample 0 by hand: h = 3, y = ((0.9 - 0.3) / (0.5 - 0.3) + 3) / 4;  w = 2, x = ((0.9 - 0.2) / (0.25 - 0.2) + 2) / 3
    y = F(F(F(F(0.9) - F(0.3)) / F(F(0.5) - F(0.3))) + F(3)) / F(4)
    x = F(F(F(F(0.9) - F(0.2)) / F(F(0.25) - F(0.2))) + F(2)) / F(3)
    assert xy[0].tolist() == [float(x), float(y)]
    assert buf_y[4:].tolist() == [guard] * 4 and buf_x[12:].tolist() == [guard] * 4 and buf_i[1:].tolist() == [guard] * 4


@pytest.fixture(scope="module")
def sampler(I, dev):
    a = I.ErrorMap(3, (5, 7), device=dev)
    a.error_map.copy_(seeded_map((3, 5, 7), 1))
    z = I.ErrorMap(3, (4, 4), device=dev)                      # a share that rounds to 0 samples
    z.error_map.copy_(seeded_map((3, 4, 4), 2))
    b = I.ErrorMap(3, (9, 4), min_pdf=0.0, device=dev)         # all mass in one cell
    b.error_map[2, 6, 1] = 5.0
    return I.ImpSampler({"a": (a, 0.3), "z": (z, 0.001), "b": (b, 0.2)}, frac_uniform=0.5)


@pytest.mark.parametrize("n", [13, 1000])
def test_imp_sampler_one_launch_equals_the_chain_segment_by_segment(I, dev, sampler, n):
    maps = list(sampler.error_maps.values())
    n_uniform, n_map = I.imp_segments(n, sampler.frac_uniform, sampler.error_map_fracs)
    assert n_map[1] == 0 and n_uniform + sum(n_map) == n and n_map[0] > 0 and n_map[2] > 0
    u = torch.rand(3, n, generator=torch.Generator().manual_seed(n)).to(dev).clamp_(1e-6, 1 - 1e-6)
    u[0, :2] = torch.tensor([1 - 1e-6, 1e-6])                  # the uniform share's ends: i = n_images - 1 and 0
    i_f, xy_f = I.imp_sample_from_uniform(maps, n_uniform, n_map, 3, u, fused=True)
    on_cpu = [types.SimpleNamespace(cdf_img=m.cdf_img.cpu(), cdf_y=m.cdf_y.cpu(), cdf_x_cond_y=m.cdf_x_cond_y.cpu()) for m in maps]
    i_c, xy_c = I.imp_sample_from_uniform(on_cpu, n_uniform, n_map, 3, u.cpu())      # true divisions (see above)
    assert i_f.shape == (n,) and xy_f.shape == (n, 2)
    b = 0
    for seg in [n_uniform] + n_map:
        assert torch.equal(i_f[b:b + seg].cpu(), i_c[b:b + seg]) and torch.equal(xy_f[b:b + seg].cpu(), xy_c[b:b + seg]), (b, seg)
        b += seg
    assert i_f[:2].tolist() == [2, 0] and torch.equal(xy_f[:n_uniform], u[1:, :n_uniform].t())
    # the map whose mass is in cell (2, 6, 1) of 9 x 4: every sample of its segment lies inside that cell
    lo = n_uniform + n_map[0]
    assert bool((i_f[lo:] == 2).all())
    x, y = xy_f[lo:, 0], xy_f[lo:, 1]
    assert bool(((x >= 1 / 4) & (x <= 2 / 4) & (y >= 6 / 9 - 1e-6) & (y <= 7 / 9 + 1e-6)).all())
    # the module draws one rand([3, n]) and makes the same call
    torch.manual_seed(77)
    i_m, xy_m = sampler.sample_img_pixel(n)
    torch.manual_seed(77)
    u = torch.rand([3, n], dtype=torch.float32, device=dev).clamp_(1e-6, 1 - 1e-6)
    i_f, xy_f = I.imp_sample_from_uniform(maps, n_uniform, n_map, 3, u, fused=True)
    assert torch.equal(i_m, i_f) and torch.equal(xy_m, xy_f)


def test_error_map_methods_take_the_fused_route(I, dev):
    m = I.ErrorMap(4, (65, 9), device=dev)
    m.error_map.copy_(seeded_map((4, 65, 9), 3))
    m.construct_cdf()
    n = 300
    frames = torch.randint(4, [n], generator=torch.Generator().manual_seed(1)).to(dev)
    for call, args in ((m.sample_img_pixel, (None, True, True)), (m.sample_img, (None, True, False)),
                       (lambda k: m.sample_pixel(k, 2), (2, False, True)), (lambda k: m.sample_pixel(k, frames), (frames, False, True))):
        torch.manual_seed(9)
        got = call(n)
        torch.manual_seed(9)
        u = torch.rand([3, n], dtype=torch.float32, device=dev).clamp_(1e-6, 1 - 1e-6)
        frame_ind, want_i, want_xy = args
        i, xy = I.errmap_sample_from_uniform(m.cdf_img, m.cdf_y, m.cdf_x_cond_y, frame_ind, u[0] if frame_ind is None else None,
                                             u[1] if want_xy else None, u[2] if want_xy else None, fused=True)
        if want_i and want_xy:
            assert torch.equal(got[0], i) and torch.equal(got[1], xy)
        else:
            assert torch.equal(got, i if want_i else xy)


# ---- update ----------------------------------------------------------------------------------------------------------------------
def run_update(I, dev, m0, i, xy, val, fused=True):
    """the update of a copy of m0 through the helper -> (the map as numpy, the scratch | None)"""
    e = torch.from_numpy(m0).to(dev)
    acc = torch.zeros(m0.shape, dtype=torch.int64, device=dev) if fused else None
    I.errmap_update(e, torch.from_numpy(i).to(dev) if isinstance(i, np.ndarray) else i, torch.from_numpy(xy).to(dev),
                    torch.from_numpy(val).to(dev), acc=acc)
    return e.cpu().numpy(), acc


@pytest.mark.parametrize("per_sample_frames", [False, True])
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 3, 130), (4, 65, 9), (1, 8, 8)])
def test_update_on_lattice_inputs_equals_chain_and_restatement(I, dev, shape, per_sample_frames):
    N, H, W = shape
    i, xy, val = ref.lattice_update(N, H, W, 5, per_sample_frames)
    assert len(val) >= 4 and not ref.cells_touched_twice(i, xy, val, N, H, W)
    m0 = (np.random.default_rng(1).integers(0, 64, shape) / 16.0).astype(F)
    want = ref.update(m0, i, xy, val)
    fused, acc = run_update(I, dev, m0, i, xy, val)
    chain, _ = run_update(I, dev, m0, i, xy, val, fused=False)
    assert not np.array_equal(want, m0)
    assert np.array_equal(fused, want) and np.array_equal(chain, want) and int(acc.abs().max()) == 0


@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 3, 130), (3, 5, 7)])
def test_update_clamps_at_the_borders(I, dev, shape):
    """x = 0, x = 1 and the last cell, and the same in y, one sample per call (so the chain is defined): x == 1 puts the whole value
    into column res_x - 2, the reference's quirk"""
    N, H, W = shape
    pts = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)]
    if shape == (1, 8, 8):
        pts += [(7.5 / 8, 0.25), (0.25, 7.5 / 8), (7.75 / 8, 7.25 / 8), (7.0 / 8, 7.0 / 8)]
    for x, y in pts:
        m0 = np.zeros(shape, F)
        xy, val = np.array([[x, y]], F), np.array([1.5], F)
        want = ref.update(m0, N - 1, xy, val)
        fused, _ = run_update(I, dev, m0, N - 1, xy, val)
        chain, _ = run_update(I, dev, m0, N - 1, xy, val, fused=False)
        assert np.array_equal(fused, want) and np.array_equal(chain, want), (x, y)
        assert float(fused.sum()) == 1.5
        if x == 1.0:
            assert fused[N - 1, :, W - 2].sum() == 1.5 and fused[N - 1, :, W - 1].sum() == 0
        if y == 1.0:
            assert fused[N - 1, H - 2, :].sum() == 1.5 and fused[N - 1, H - 1, :].sum() == 0


@pytest.mark.parametrize("case", ["one_cell", "random"])
def test_update_accumulates_collisions_reproducibly(I, dev, case):
    shape = (3, 5, 7)
    rng = np.random.default_rng(2)
    if case == "one_cell":                                     # 257 samples into ONE cell (all four corners shared)
        n = 257
        i = 1
        xy = (np.array([2 / 7, 3 / 5]) + rng.random((n, 2)) * np.array([0.9 / 7, 0.9 / 5])).astype(F)
    else:                                                      # 4096 samples on 105 cells: almost all collide
        n = 4096
        i = rng.integers(0, 3, n)
        xy = rng.random((n, 2)).astype(F)
    val = rng.random(n).astype(F)
    m0 = np.zeros(shape, F)
    want, counts, exact = ref.update(m0, i, xy, val, return_counts=True)
    got, acc = run_update(I, dev, m0, i, xy, val)
    again, _ = run_update(I, dev, m0, i, xy, val)
    assert counts.max() >= (257 if case == "one_cell" else 100)
    assert got.tobytes() == want.tobytes() and again.tobytes() == got.tobytes()
    assert int(acc.abs().max()) == 0                           # the scratch is all zero afterwards
    bound = counts * 2.0 ** -33 + 2.0 ** -24 * np.abs(exact)
    err = np.abs(got.astype(np.float64) - exact)
    print(f"update {case}: largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert np.all(err <= bound)
    # ... and through the module on a map that is not zero: the scratch is the module's own, zero again, the result the restatement's
    m = I.ErrorMap(3, (5, 7), device=dev)
    m.error_map.copy_(seeded_map(shape, 4))
    start = m.error_map.cpu().numpy().copy()
    m.update_error_map(torch.from_numpy(i).to(dev) if case == "random" else i, torch.from_numpy(xy).to(dev), torch.from_numpy(val).to(dev))
    assert m._update_acc is not None and int(m._update_acc.abs().max()) == 0 and list(m.state_dict()) == ["error_map"]
    assert np.array_equal(m.error_map.cpu().numpy(), ref.update(start, i, xy, val))


def test_update_drops_bad_samples(I, dev):
    m0 = seeded_map((3, 5, 7), 8).numpy()
    xy = np.array([[0.5, 0.5], [0.5, 0.5], [np.nan, 0.5], [0.5, np.inf], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5]], F)
    val = np.array([1.0, 1.0, 1.0, 1.0, np.inf, np.nan, -1.0], F)
    i = np.array([-1, 3, 0, 1, 2, 0, 1], np.int64)
    got, acc = run_update(I, dev, m0, i, xy, val)
    assert got.tobytes() == m0.tobytes() and int(acc.abs().max()) == 0
    for frame in (-1, 3):                                      # the same with a scalar frame
        got, _ = run_update(I, dev, m0, frame, xy[:1], val[:1])
        assert got.tobytes() == m0.tobytes()
    # a good sample among them is still applied
    i[1] = 2
    got, _ = run_update(I, dev, m0, i, xy, val)
    assert np.array_equal(got, ref.update(m0, i, xy, val)) and not np.array_equal(got, m0)


def test_update_splits_long_calls_into_chunks(I, dev):
    """40 000 samples into one cell: two chunks of at most 2^15, each a scatter plus an apply, in order"""
    n = 40000
    rng = np.random.default_rng(3)
    xy = np.tile(np.array([[0.3, 0.3]], F), (n, 1))
    val = rng.random(n).astype(F)
    m0 = np.zeros((1, 4, 4), F)
    got, acc = run_update(I, dev, m0, 0, xy, val)
    assert np.array_equal(got, ref.update(m0, 0, xy, val)) and int(acc.abs().max()) == 0
    assert got.sum() > 0.49 * n * 0.99


# ---- construct_cdf ---------------------------------------------------------------------------------------------------------------
CDF_CONFIGS = [dict(min_pdf=0.01), dict(min_pdf=0.0), dict(min_pdf=0.01, max_pdf=0.7)]
_worst = {"fraction": 0.0}


@pytest.mark.parametrize("N,H", [(1, 3), (1, 65), (70, 3), (70, 65)])
@pytest.mark.parametrize("W", [7, 64, 65, 128, 129, 130])
def test_construct_cdf_equals_the_restatement(B, dev, N, H, W):
    e0 = seeded_map((N, H, W), 100 + W).numpy()
    for kw in CDF_CONFIGS:
        want = ref.construct_cdf(e0, **kw)
        exact = ref.construct_cdf_f64(e0, **kw)
        e = torch.from_numpy(e0.copy()).to(dev)
        got = B.construct_cdf(e, kw["min_pdf"], kw.get("max_pdf"))
        assert np.array_equal(e.cpu().numpy(), want[3])                            # clamped in place with max_pdf, untouched without
        for name, g, w, x in zip(("cdf_x_cond_y", "cdf_y", "cdf_img"), got, want, exact):
            g = g.cpu().numpy()
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (name, kw)
            assert np.all(np.diff(g, axis=-1) >= 0), name
            assert np.all(np.abs(g[..., -1].astype(np.float64) - 1) <= 2.0 ** -23), name
            L = g.shape[-1]
            bound = (9 + math.ceil(L / 64)) * 2.0 ** -24
            frac = float((np.abs(g - x) / (bound * np.abs(x))).max())
            _worst["fraction"] = max(_worst["fraction"], frac)
            assert frac <= 1, (name, kw, frac)
        e = torch.from_numpy(e0.copy()).to(dev)
        clean = B.construct_cdf(e, kw["min_pdf"], kw.get("max_pdf"), clean=True)
        assert all(torch.equal(a, b) for a, b in zip(clean, got)) and int((e != 0).sum()) == 0
    print(f"construct_cdf {N}x{H}x{W}: largest error / bound so far = {_worst['fraction']:.3f}")


def test_module_construct_cdf_takes_the_fused_route(I, B, dev):
    m = I.ErrorMap(2, (3, 130), min_pdf=0.01, max_pdf=0.7, device=dev)
    e0 = seeded_map((2, 3, 130), 9)
    m.error_map.copy_(e0)
    m.construct_cdf()
    want = ref.construct_cdf(e0.numpy(), 0.01, 0.7)
    for a, w in zip((m.cdf_x_cond_y, m.cdf_y, m.cdf_img, m.error_map), want):
        assert np.array_equal(a.cpu().numpy(), w)
    m.construct_cdf_and_clean_error_map()
    assert int((m.error_map != 0).sum()) == 0
    # the chain on the same map: the same CDFs up to the order of torch's own cumsum
    m2 = I.ErrorMap(2, (3, 130), min_pdf=0.01, max_pdf=0.7, device=dev)
    m2.error_map.copy_(e0)
    saved = I.FUSED_IMPORTANCE
    I.FUSED_IMPORTANCE = False
    try:
        m2.construct_cdf()
    finally:
        I.FUSED_IMPORTANCE = saved
    for a, b in zip((m.cdf_x_cond_y, m.cdf_y, m.cdf_img), (m2.cdf_x_cond_y, m2.cdf_y, m2.cdf_img)):
        torch.testing.assert_close(a, b, rtol=2e-6, atol=0)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_max", [("max", 50), ("nomax", None)])
def test_step_error_map_schedule_and_sampling(I, dev, name, n_max):
    sched = np.load(os.path.join(ROOT, "tests", "golden", "ref_importance.npz"))[f"schedule/{name}"]
    N = 5
    m = I.ErrorMap(N, (16, 24), n_steps_init=8, n_steps_max=n_max, device=dev)
    g = torch.Generator().manual_seed(0)
    for s in range(200):
        frames = torch.randint(N, [256], generator=g).to(dev)
        m.step_error_map(frames if s % 2 else s % N, torch.rand(256, 2, generator=g).to(dev), torch.rand(256, generator=g).to(dev))
    assert (m.n_steps_between_update, m.n_steps_since_update) == tuple(sched[199].tolist())
    assert m.cdf_img is not None and int(m._update_acc.abs().max()) == 0
    i, xy = m.sample_img_pixel(1000)
    assert i.shape == (1000,) and i.dtype == torch.int64 and int(i.min()) >= 0 and int(i.max()) < N
    assert xy.shape == (1000, 2) and bool((xy > 0).all()) and bool((xy < 1).all())
