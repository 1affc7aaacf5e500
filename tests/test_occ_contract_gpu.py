"""GPU: the tanh / sphere contracted occupancy march (csrc/occ_grid.hip: contract<>, probe<>, the `else` arm of march_ray_group, the
second march k_march<true, false>) -- every probe judged, only proven ties excused.

Outside AABB grids a ray's probe sequence does not depend on what is probed, so
  (a) a march through an all-ones grid with the cap above the longest ray lists every probe (the *trace*): packed_info, t_starts,
      t_ends and ridx equal the oracle's bit for bit; the sphere's cells too (every operation correctly rounded on both sides); a tanh
      cell is the float64 cell (tests/occ_contract_ref.py), or on a probe within the derived tie distance of a voxel face the cell
      across that face;
  (b) a march through any grid with any cap is EXACTLY "the first `cap` probes of the device's own trace whose cell is occupied",
      whatever tanhf did -- the check of the look-ahead's ballot, slot and cap logic, with caps inside a group of 16 / 32 / 64 lanes;
  (c) every ray without an undecided probe equals the oracle on all five outputs;
  (d) the second march, the batched marcher, ray_marching_finished, the occgrid_raymarch wrapper and ray_marching_composite give the
      same samples;  (e) zero rays.
The scenes and their preconditions: tests/occ_contract_inputs.py, tests/test_occ_contract_cpu.py."""
import numpy as np
import pytest
import torch

import occ_contract_inputs as I
import occ_contract_ref as R

pytestmark = pytest.mark.gpu
NAMES5 = ["packed_info", "t_starts", "t_ends", "ridx", "gidx"]
NAMES6 = ["packed_info", "t_starts", "t_ends", "ridx", "bidx", "gidx"]


@pytest.fixture(autouse=True, params=["1", "16", "32", "64"], ids=lambda v: f"lanes_per_ray={v}")
def march_group(request, hip_option):
    """every test under each count pass: one lane per ray (k_march) and 16 / 32 / 64 lanes per ray (k_march_group) -- the same bits"""
    hip_option("march_group", request.param)
    return request.param


_RAYS, _ORACLE, _DEVICE = {}, {}, {}


def on_dev(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rays_on(dev, key, sc):
    if key not in _RAYS:
        _RAYS[key] = tuple(on_dev(dev, sc[k]) for k in ("o", "d", "near", "far"))
    return _RAYS[key]


def host(outs):
    return [None if t is None else t.cpu().numpy() for t in outs]


def device_march(dev, group, name, ctype, kind, cap):
    """the library's march of a scene (numpy outputs), computed once per lanes-per-ray setting and shared; kind 'full' with the cap
    TRACE_STEPS is the trace"""
    from nr3d_lib_amd.bindings import _occ_grid
    key = (group, name, ctype, kind, cap)
    if key not in _DEVICE:
        sc = I.scene(name)
        grid = np.ones(sc["res"], bool) if kind == "full" else I.scene_grids(sc["res"])[kind]
        _DEVICE[key] = host(_occ_grid.ray_marching(*rays_on(dev, name, sc), on_dev(dev, sc["roi"]), on_dev(dev, grid),
                                                   _occ_grid.ContractionType(ctype), sc["step"], sc["max_step"], sc["gamma"], cap, True))
    return _DEVICE[key]


def oracle_march(oracle, name, ctype, kind, cap):
    key = (name, ctype, kind, cap)
    if key not in _ORACLE:
        sc = I.scene(name)
        grid = np.ones(sc["res"], bool) if kind == "full" else I.scene_grids(sc["res"])[kind]
        _ORACLE[key] = oracle.ray_marching(sc["o"], sc["d"], sc["near"], sc["far"], *I.march_args(sc, grid, ctype, cap))
    return _ORACLE[key]


def verdict(oracle, name, ctype):
    """the float64 judge on the scene's probes (the trace's t values are the same on both sides: asserted by test_trace_parity)"""
    key = (name, ctype, "judge")
    if key not in _ORACLE:
        sc, tr = I.scene(name), oracle_march(oracle, name, ctype, "full", I.TRACE_STEPS)
        _ORACLE[key] = R.judge(sc["o"], sc["d"], sc["roi"], sc["res"], ctype, tr[1], tr[2], tr[3])
    return _ORACLE[key]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def assert_packed(outs, n, names):
    """dtypes and shapes of a marcher's list, and packs that tile the samples in ray order"""
    pi, S = outs[0], outs[1].shape[0]
    assert pi.dtype == np.int32 and pi.shape == (n, 2)
    assert outs[1].dtype == np.float32 and outs[1].shape == (S, 1) and outs[2].dtype == np.float32 and outs[2].shape == (S, 1)
    for a, nm in zip(outs[3:], names[3:]):
        assert a.dtype == np.int32 and a.shape == (S,), nm
    assert (pi[:, 0] == np.cumsum(pi[:, 1]) - pi[:, 1]).all() and int(pi[:, 1].sum()) == S
    assert (outs[3] == np.repeat(np.arange(n, dtype=np.int32), pi[:, 1])).all(), "ridx"


def assert_rays_equal(got, want, rays, names, what):
    """the rays of the mask `rays` have the same count and the same samples in both results"""
    assert (got[0][rays, 1] == want[0][rays, 1]).all(), f"{what}: sample counts of {int((got[0][rays, 1] != want[0][rays, 1]).sum())} rays differ"
    mg, mw = rays[got[3]], rays[want[3]]
    for g, w, nm in zip(got[1:], want[1:], names[1:]):
        assert same_bits(g[mg], w[mw]), f"{what}: {nm} differs"


SCENE_CASES = [(name, ctype) for name in I.SCENES for ctype in I.CTYPES]


@pytest.mark.parametrize("name,ctype", SCENE_CASES)
def test_trace_parity(oracle, dev, march_group, name, ctype):
    sc = I.scene(name)
    n = sc["o"].shape[0]
    got = device_march(dev, march_group, name, ctype, "full", I.TRACE_STEPS)
    want = oracle_march(oracle, name, ctype, "full", I.TRACE_STEPS)
    assert_packed(got, n, NAMES5)
    assert got[0][:, 1].max() < I.TRACE_STEPS
    for g, w, nm in zip(got[:4], want[:4], NAMES5):                   # independent of the contraction: always bit-equal
        assert same_bits(g, w), f"{nm} differs from the oracle's ({g.shape} vs {w.shape})"
    j = verdict(oracle, name, ctype)
    differs = int((got[4] != want[4]).sum())
    if ctype == R.SPHERE:
        print(f"\nEXCUSED {name} sphere lanes {march_group}: 0 (nothing is excused), {differs} cells differ from the oracle")
        assert differs == 0, f"sphere: {differs} of {got[4].shape[0]} cells differ from the oracle"
        return
    bad, excused = R.check_cells(j, got[4], sc["res"])
    print(f"\nEXCUSED {name} tanh lanes {march_group}: {int(excused.sum())} of {bad.shape[0]} probes ({int(j['undecided'].any(1).sum())} undecided), "
          f"{differs} cells differ from the oracle")
    assert not bad.any(), (f"tanh: {int(bad.sum())} of {bad.shape[0]} probes are neither in the float64 cell nor within the tie distance of the "
                           f"face they crossed ({int(excused.sum())} excused); first: probe {int(np.nonzero(bad)[0][0])}")


@pytest.mark.parametrize("name,ctype", SCENE_CASES)
def test_filter_identity(dev, march_group, name, ctype):
    """exact, no tolerance: the march == the first `cap` occupied probes of the device's own trace"""
    sc = I.scene(name)
    n = sc["o"].shape[0]
    trace = device_march(dev, march_group, name, ctype, "full", I.TRACE_STEPS)
    for kind, grid in I.scene_grids(sc["res"]).items():
        for cap in I.CAPS:
            got = device_march(dev, march_group, name, ctype, kind, cap)
            want = R.filter_trace(trace, grid, cap, n)
            assert_packed(got, n, NAMES5)
            for g, w, nm in zip(got, want, NAMES5):
                assert same_bits(g, w), f"{kind} cap {cap}: {nm} is not the filtered trace ({g.shape} vs {w.shape})"


@pytest.mark.parametrize("name,ctype", SCENE_CASES)
def test_against_oracle(oracle, dev, march_group, name, ctype):
    """every ray without an undecided probe (sphere: every ray) equals the oracle on all five outputs"""
    sc = I.scene(name)
    n = sc["o"].shape[0]
    j = verdict(oracle, name, ctype)
    trace = oracle_march(oracle, name, ctype, "full", I.TRACE_STEPS)
    clean = np.ones(n, bool) if ctype == R.SPHERE else ~R.ray_has(j["undecided"].any(1), trace[3], n)
    assert clean.mean() >= 0.9
    for kind in I.scene_grids(sc["res"]):
        for cap in I.CAPS:
            got = device_march(dev, march_group, name, ctype, kind, cap)
            want = oracle_march(oracle, name, ctype, kind, cap)
            assert_rays_equal(got, want, clean, NAMES5, f"{kind} cap {cap}")
            if clean.all():
                assert same_bits(got[0], want[0]), f"{kind} cap {cap}: packed_info"


# ---- (d) routes, on the non-power-of-two scene ----------------------------------------------------------------------------------
ROUTE_CAPS = (7, 65, I.TRACE_STEPS)


@pytest.mark.parametrize("ctype", I.CTYPES)
def test_second_march_gives_the_cached_tensors(dev, march_group, monkeypatch, ctype):
    """SAMPLE_CACHE_MAX_BYTES = 0: count without the cache, then k_march<true, false> with max_steps from packed_info"""
    from nr3d_lib_amd.bindings import _occ_grid
    sc = I.scene("non_pow2")
    for kind in ("full", "random", "shell"):
        grid = np.ones(sc["res"], bool) if kind == "full" else I.scene_grids(sc["res"])[kind]
        for cap in ROUTE_CAPS:
            cached = device_march(dev, march_group, "non_pow2", ctype, kind, cap)
            with monkeypatch.context() as m:
                m.setattr(_occ_grid, "SAMPLE_CACHE_MAX_BYTES", 0)
                twice = host(_occ_grid.ray_marching(*rays_on(dev, "non_pow2", sc), on_dev(dev, sc["roi"]), on_dev(dev, grid),
                                                    _occ_grid.ContractionType(ctype), sc["step"], sc["max_step"], sc["gamma"], cap, True))
            for a, b, nm in zip(cached, twice, NAMES5):
                assert same_bits(a, b), f"{kind} cap {cap}: {nm}"


@pytest.mark.parametrize("case", ["batch_inds", "batch_data_size"])
@pytest.mark.parametrize("ctype", I.CTYPES)
def test_batched(oracle, dev, march_group, ctype, case):
    """three grids over three ROIs (one power of two, two not): the trace against the oracle and the judge per entry, then the filter
    identity and the oracle on the undisputed rays, bidx included"""
    from nr3d_lib_amd.bindings import _occ_grid
    sc, kw = I.batch_cases()[case]
    n, vol = sc["o"].shape[0], int(np.prod(I.BATCH_RES))
    r = rays_on(dev, ("batched", case), sc)
    roi_t, bi_t = on_dev(dev, I.BATCH_ROI), on_dev(dev, kw.get("batch_inds"))

    def both(grid, cap):
        got = host(_occ_grid.batched_ray_marching(*r, bi_t, kw.get("batch_data_size"), roi_t, on_dev(dev, grid), _occ_grid.ContractionType(ctype),
                                                  sc["step"], sc["max_step"], sc["gamma"], cap, True))
        want = oracle.ray_marching(sc["o"], sc["d"], sc["near"], sc["far"], I.BATCH_ROI, grid, ctype, sc["step"], sc["max_step"], sc["gamma"],
                                   cap, True, **kw)
        assert_packed(got, n, NAMES6)
        return got, want

    trace, otrace = both(I.batch_grids("full"), I.TRACE_STEPS)
    for g, w, nm in zip(trace[:5], otrace[:5], NAMES6):
        assert same_bits(g, w), f"trace {nm}"
    assert (trace[5] // vol == trace[4]).all(), "gidx carries the entry's offset"
    if "batch_inds" in kw:
        assert (trace[0][kw["batch_inds"] < 0, 1] == 0).all()
    j = R.judge(sc["o"], sc["d"], I.BATCH_ROI[trace[4]], I.BATCH_RES, ctype, trace[1], trace[2], trace[3])
    if ctype == R.SPHERE:
        assert same_bits(trace[5], otrace[5]), "sphere: cells differ from the oracle"
        clean = np.ones(n, bool)
    else:
        bad, excused = R.check_cells(j, trace[5] - trace[4] * vol, I.BATCH_RES)
        print(f"\nEXCUSED batched/{case} tanh lanes {march_group}: {int(excused.sum())} of {bad.shape[0]} probes")
        assert not bad.any(), f"tanh: {int(bad.sum())} probes outside the tie distance ({int(excused.sum())} excused)"
        clean = ~R.ray_has(j["undecided"].any(1), trace[3], n)
    grid = I.batch_grids("random")
    for cap in (7, 40, 65, I.TRACE_STEPS):
        got, want = both(grid, cap)
        for g, w, nm in zip(got, R.filter_trace(trace, grid, cap, n), NAMES6):
            assert same_bits(g, w), f"cap {cap}: {nm} is not the filtered trace"
        assert_rays_equal(got, want, clean, NAMES6, f"cap {cap}")


@pytest.mark.parametrize("ctype", I.CTYPES)
def test_finished_and_wrapper(dev, march_group, ctype):
    """ray_marching_finished == the fields derived from ray_marching's outputs (as test_fused_march_finish_against_chain does for AABB);
    occgrid_raymarch(constraction=...) returns that record"""
    from nr3d_lib_amd.bindings import _occ_grid
    from nr3d_lib_amd.graphics.raymarch.occgrid_raymarch import occgrid_raymarch
    sc = I.scene("non_pow2")
    n = sc["o"].shape[0]
    o, d, near, far = rays_on(dev, "non_pow2", sc)
    roi, grid = on_dev(dev, sc["roi"]), on_dev(dev, I.scene_grids(sc["res"])["random"])
    for cap in ROUTE_CAPS:
        pi, ts, te, ridx, gidx = device_march(dev, march_group, "non_pow2", ctype, "random", cap)
        m = _occ_grid.ray_marching_finished(o, d, near, far, roi, grid, _occ_grid.ContractionType(ctype), sc["step"], sc["max_step"], sc["gamma"],
                                            cap, True)
        hit = np.nonzero(pi[:, 1])[0]
        assert m["n_hit"] == len(hit) > 0 and m["bidx"] is None
        want = dict(ridx_hit=hit.astype(np.int64), pack_infos=pi[hit].astype(np.int64), t_starts=ts[:, 0], t_ends=te[:, 0],
                    ridx=ridx.astype(np.int64), deltas=te[:, 0] - ts[:, 0], gidx=gidx)
        for k, w in want.items():
            g = m[k].cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.int32), w.view(np.int32)), f"cap {cap}: {k}"
        # samples = fmaf(d, t, o), one rounding: equal to the exactly rounded value, and within one ulp of |position| < 8 (1e-6, the
        # bound of the AABB test) of the twice-rounded chain o + d * t
        samples = m["samples"].cpu().numpy()
        assert samples.dtype == np.float32 and samples.shape == (ts.shape[0], 3)
        assert same_bits(samples, R.fma32(sc["d"][ridx], ts, sc["o"][ridx])), f"cap {cap}: samples"
        chain = torch.addcmul(o.index_select(0, m["ridx"]), d.index_select(0, m["ridx"]), m["t_starts"].unsqueeze(-1))
        assert float((m["samples"] - chain).abs().max()) <= 1e-6 and float(chain.abs().max()) < 8
        ret = occgrid_raymarch(grid, o, d, near, far, constraction={1: "tanh", 2: "sphere"}[ctype], roi=roi, step_size=sc["step"],
                               max_step_size=sc["max_step"], dt_gamma=sc["gamma"], max_steps=cap)
        assert ret.num_hit_rays == m["n_hit"]
        for field, k in (("ridx_hit", "ridx_hit"), ("samples", "samples"), ("depth_samples", "t_starts"), ("deltas", "deltas"),
                         ("ridx", "ridx"), ("pack_infos", "pack_infos")):
            assert torch.equal(getattr(ret, field), m[k]), f"cap {cap}: wrapper {field}"
        assert ret.gidx.dtype == torch.int64 and torch.equal(ret.gidx, m["gidx"].long())
    with pytest.raises(RuntimeError, match="constraction"):
        occgrid_raymarch(grid, o, d, near, far, constraction="cube", roi=roi)


def test_march_composite_tanh(dev, march_group):
    """ray_marching_composite through a tanh-contracted grid == ray_marching_finished + tau_to_alpha + packed_composite_forward on the
    same samples, bit for bit (forward; the AABB test test_march_composite_in_one_call also runs the backward)"""
    from nr3d_lib_amd.bindings import _occ_grid, _pack_ops
    sc = I.scene("non_pow2")
    n, cap = sc["o"].shape[0], 65
    o, d, near, far = rays_on(dev, "non_pow2", sc)
    roi, grid = on_dev(dev, sc["roi"]), on_dev(dev, I.scene_grids(sc["res"])["random"])
    args = (o, d, near, far, roi, grid, _occ_grid.ContractionType.UN_BOUNDED_TANH, sc["step"], sc["max_step"], sc["gamma"], cap)
    m = _occ_grid.ray_marching_finished(*args, True)
    S = m["t_starts"].shape[0]
    rng = np.random.default_rng(11)
    sigma = on_dev(dev, (10.0 * rng.random(S + 5) ** 2).astype(np.float32))
    rgb = on_dev(dev, rng.random((S + 5, 3), dtype=np.float32))
    out = _occ_grid.ray_marching_composite(*args, sigma, rgb, 1e-4, 0.02, True).result()
    pi = device_march(dev, march_group, "non_pow2", 1, "random", cap)[0]
    assert out["n_hit"] == m["n_hit"] > 0 and same_bits(out["packed_info"].cpu().numpy(), pi)
    for k in ("ridx_hit", "pack_infos", "t_starts", "t_ends", "ridx", "deltas", "samples", "gidx"):
        assert out[k].dtype == m[k].dtype and torch.equal(out[k], m[k]), k
    alpha = _pack_ops.tau_to_alpha_forward(sigma[:S].contiguous(), m["deltas"])
    vw, mask, depth, col = _pack_ops.packed_composite_forward(alpha, m["t_starts"], rgb[:S].contiguous(), m["pack_infos"], m["ridx_hit"], n,
                                                              1e-4, 0.02, True, packs_tile=True)
    for k, w in (("alpha", alpha), ("vw", vw), ("mask", mask), ("depth", depth), ("rgb", col)):
        assert torch.equal(out[k].view(torch.int32), w.view(torch.int32)), k
    assert float(mask.sum()) > 0


# ---- (e) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", I.CTYPES)
def test_zero_rays(dev, ctype):
    from nr3d_lib_amd.bindings import _occ_grid
    e3, e1 = torch.empty((0, 3), device=dev), torch.empty(0, device=dev)
    ct = _occ_grid.ContractionType(ctype)
    grid = on_dev(dev, np.ones((8, 8, 8), bool))
    out = _occ_grid.ray_marching(e3, e3, e1, e1, on_dev(dev, I.ROI_POW2), grid, ct, 0.02, 1e10, 0.0, 64, True)
    assert [tuple(t.shape) for t in out] == [(0, 2), (0, 1), (0, 1), (0,), (0,)]
    assert [t.dtype for t in out] == [torch.int32, torch.float32, torch.float32, torch.int32, torch.int32]
    outb = _occ_grid.batched_ray_marching(e3, e3, e1, e1, torch.empty(0, dtype=torch.int32, device=dev), None, on_dev(dev, I.BATCH_ROI),
                                          on_dev(dev, np.ones((3, 8, 8, 8), bool)), ct, 0.02, 1e10, 0.0, 64, True)
    assert [tuple(t.shape) for t in outb] == [(0, 2), (0, 1), (0, 1), (0,), (0,), (0,)]
    assert [t.dtype for t in outb] == [torch.int32, torch.float32, torch.float32] + [torch.int32] * 3
    m = _occ_grid.ray_marching_finished(e3, e3, e1, e1, on_dev(dev, I.ROI_POW2), grid, ct, 0.02, 1e10, 0.0, 64, True)
    assert m["n_hit"] == 0 and tuple(m["samples"].shape) == (0, 3) and tuple(m["pack_infos"].shape) == (0, 2)
    assert (m["ridx_hit"].dtype, m["pack_infos"].dtype, m["ridx"].dtype, m["gidx"].dtype) == (torch.int64, torch.int64, torch.int64, torch.int32)
    assert all(tuple(m[k].shape) == (0,) for k in ("ridx_hit", "t_starts", "t_ends", "ridx", "deltas", "gidx"))
