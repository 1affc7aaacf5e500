"""GPU: the fused NeRF++ shell marcher (csrc/nerfpp_march.hip through bindings._nerfpp_march and graphics/raymarch/nerfpp_raymarch.py
with fused=True) against the float64 restatement of tests/nerfpp_march_ref.py and against the project's torch chain (fused=False) on
the same device.

Integers (ridx_hit, pack_infos, ridx) are EQUAL to the chain's and to the float64 restatement's, no case excused: every ray set has
``near_ties == 0`` (asserted, on the very radii and noise the routes use), so no validity decision is close enough for float32 and
float64 to differ.  Floats go by the yardstick of tests/test_neus_alpha_gpu.py: the error against float64, relative to the tensor's
maximum, is at most 4 x the chain's own float32 error on the same inputs, and a larger ratio passes only while the error is below
1e-5 of the maximum.  Why 4: both routes evaluate the same float32 expressions with IEEE division and square root; they differ in
pow / log10, in the order of the three-term sums and in the rounding of the normalised ray.  With include_inf_distance the last shell's
delta is of order 1e10 and would hide every other delta behind the maximum: those entries are judged by their relative error, element
by element, with the same rule.  Every check prints its ratio ("YARDSTICK ..."); tools/exp_nerfpp_march.py --yardstick folds a log of
them into profiles/nerfpp_march.json, which keeps one run: 3456 checks here, the largest ratios 3.9 (samples), 2.0 (depth_samples),
1.0 (deltas to the far shell) and, for deltas, 4.52 at an error of 1.9e-07, below the 1e-5 floor."""
import functools

import pytest
import torch

import nerfpp_march_ref as ref

pytestmark = pytest.mark.gpu

R_MIN, R_MAX = 1.0, 100.0
RAYS = (1, 5, 67)
TABLE_LENGTHS = (1, 8, 63, 64, 65, 101, 256)
SEEDS = {1: 3, 5: 1, 67: 896}                   # ray-set seeds with near_ties == 0 on every table (test_nerfpp_march_cpu.py)
SEED_INSIDE = 0
FIELDS_INT = ("ridx_hit", "pack_infos", "ridx")
NOISE_SEED = 1234


@functools.lru_cache(maxsize=None)
def steps_for(interval, n):
    """the max_steps whose table has n entries (arange decides: max_steps or one more)"""
    for steps in (n, n - 1):
        if steps >= 1 and ref.shell_table(R_MIN, R_MAX, steps, interval)[0].numel() == n:
            return steps
    raise AssertionError(f"no max_steps gives a table of {n} for {interval}")


def all_ray_sets():
    """(R, seed, kind, interval type, max_steps, include_inf_distance) of every ray set the GPU tests march, for the CPU test of the
    input condition (the third interval type shares the logarithm's geometry)"""
    out = []
    for R in RAYS:
        for n in TABLE_LENGTHS:
            for interval in ref.INTERVALS[:2]:
                for inf in (False, True):
                    out.append((R, SEEDS[R], "mixed", interval, steps_for(interval, n), inf))
    for interval in ref.INTERVALS[:2]:
        out += [(67, SEEDS[67], kind, interval, 33, True) for kind in ("mixed", "empty_edges")] + [(67, SEED_INSIDE, "inside", interval, 33, True)]
    return sorted(set(out))


def _march(dev, case, mode, interval, steps, inf, perturb, fused, seed=NOISE_SEED):
    from nr3d_lib_amd.graphics.raymarch import nerfpp_raymarch
    from nr3d_lib_amd.models.spatial import AABBSpace
    aabb, o, d, t_min = case
    torch.manual_seed(seed)
    ret = nerfpp_raymarch(AABBSpace(aabb=aabb, device=dev), o, d, t_min, None, radius_scale_min=R_MIN, radius_scale_max=R_MAX,
                          include_inf_distance=inf, perturb=perturb, max_steps=steps, sample_mode=mode, interval_type=interval, fused=fused)
    return ret, torch.cuda.get_rng_state(dev)


@functools.lru_cache(maxsize=None)
def _case(R, seed, kind):
    dev = torch.device("cuda:0")
    return tuple(t.to(dev) for t in ref.rays(R, seed, kind))


def _inputs(dev, case, interval, steps, inf, perturb):
    """the table, and the noise both routes draw -- from the first seed at which no decision is near a tie"""
    radii, step, lo, hi = ref.shell_table(R_MIN, R_MAX, steps, interval, device=dev)
    last = ref.last_radius(R_MAX, inf)
    for seed in range(NOISE_SEED, NOISE_SEED + (8 if perturb else 1)):
        torch.manual_seed(seed)
        noise = torch.rand([case[1].shape[0], radii.numel()], device=dev) if perturb else None
        ties = [ref.near_ties(*case, radii, noise, step, last, mode, interval) for mode in ref.MODES]
        if sum(ties) == 0:
            return seed, radii, noise, step, last, lo, hi
    raise AssertionError(f"input condition: near ties {ties} at every seed tried")


def _yardstick(name, got, r64, r32, relative=False):
    assert torch.equal(torch.isnan(got), torch.isnan(r64)), f"{name}: NaN in other places than the float64 evaluation"
    keep = ~torch.isnan(r64)
    got, r64, r32 = got[keep].double(), r64[keep], r32[keep].double()
    if got.numel() == 0:
        return
    assert torch.isfinite(got).all(), f"{name}: not finite"
    scale = r64.abs() if relative else (float(r64.abs().max()) or 1.0)
    err = float(((got - r64).abs() / scale).max())
    err32 = float(((r32 - r64).abs() / scale).max())
    print(f"YARDSTICK {name}: rel err {err:.3e} torch fp32 {err32:.3e} ratio {err / err32 if err32 else float('inf'):.2f}")
    assert err <= max(1e-5, 4 * err32), f"{name}: rel err {err:.2e} (torch fp32 chain: {err32:.2e})"


def _compare(tag, fused, chain, r64, n_table, inf):
    if r64 is None:
        assert all(v is None for v in fused) and all(v is None for v in chain), f"{tag}: expected no sample"
        return
    for f in FIELDS_INT:
        a, b, c = getattr(fused, f), getattr(chain, f), r64[f]
        assert a.dtype == torch.int64 and a.shape == b.shape and torch.equal(a, b), f"{tag} {f}: differs from the chain"
        assert torch.equal(a, c), f"{tag} {f}: differs from the float64 evaluation"
    _yardstick(f"{tag} samples", fused.samples, r64["samples"], chain.samples)
    _yardstick(f"{tag} depth_samples", fused.depth_samples, r64["depth_samples"], chain.depth_samples)
    last = (r64["pidx"] == n_table - 1) if inf else torch.zeros_like(r64["pidx"], dtype=torch.bool)
    _yardstick(f"{tag} deltas", fused.deltas[~last], r64["deltas"][~last], chain.deltas[~last])
    if bool(last.any()):
        _yardstick(f"{tag} deltas to the far shell", fused.deltas[last], r64["deltas"][last], chain.deltas[last], relative=True)


@pytest.mark.parametrize("R", RAYS)
@pytest.mark.parametrize("interval", ref.INTERVALS)
@pytest.mark.parametrize("mode", ref.MODES)
def test_fused_matches_float64_and_the_chain(dev, mode, interval, R):
    case = _case(R, SEEDS[R], "mixed")
    for n in TABLE_LENGTHS:
        steps = steps_for(interval, n)
        for inf in (False, True):
            for perturb in (False, True):
                seed, radii, noise, step, last, lo, hi = _inputs(dev, case, interval, steps, inf, perturb)
                assert radii.numel() == n
                fused, state_f = _march(dev, case, mode, interval, steps, inf, perturb, True, seed)
                chain, state_c = _march(dev, case, mode, interval, steps, inf, perturb, False, seed)
                assert torch.equal(state_f, state_c), "the two routes leave the generator in different states"
                r64 = ref.march(*case, radii, noise, step, last, mode, interval, lo, hi, dtype=torch.float64)
                _compare(f"{mode} {interval} R {R} N {n} inf {int(inf)} perturb {int(perturb)}", fused, chain, r64, n, inf)


@pytest.mark.parametrize("mode", ref.MODES)
def test_rays_without_samples(dev, mode):
    """all rays cut off: six None; rays cut off in front, in the middle and at the end: the chain's ridx_hit"""
    none, _ = _march(dev, _case(5, SEEDS[5], "none"), mode, "inverse_proportional", 33, True, False, True)
    assert tuple(none) == (None,) * 6
    case = _case(67, SEEDS[67], "empty_edges")
    fused, _ = _march(dev, case, mode, "inverse_proportional", 33, True, False, True)
    chain, _ = _march(dev, case, mode, "inverse_proportional", 33, True, False, False)
    for f in FIELDS_INT:
        assert torch.equal(getattr(fused, f), getattr(chain, f)), f
    hit = set(fused.ridx_hit.tolist())
    assert not hit & {0, 1, 33, 34, 65, 66} and len(hit) > 8
    assert fused.pack_infos[-1].sum().item() == fused.ridx.numel() == fused.samples.shape[0]
    from nr3d_lib_amd import _hip
    assert _hip.tiles(fused.pack_infos, fused.ridx.numel())


@pytest.mark.parametrize("mode", ["box", "cube"])
def test_ray_on_a_face_plane_loses_that_shell(dev, mode):
    """0 / 0 in a slab: NaN through min / max, the shell is invalid on both routes (fminf / fmaxf would have kept it)"""
    from nr3d_lib_amd.graphics.raymarch import nerfpp_raymarch
    from nr3d_lib_amd.models.spatial import AABBSpace
    aabb, o, d, t_min, kw = ref.face_plane_case()
    aabb, o, d, t_min = (t.to(dev) for t in (aabb, o, d, t_min))
    radii, step, lo, hi = ref.shell_table(kw["radius_scale_min"], kw["radius_scale_max"], kw["max_steps"], kw["interval_type"])
    assert radii.tolist() == [1.0, 0.875, 0.75, 0.625, 0.5, 0.375]
    outs = [nerfpp_raymarch(AABBSpace(aabb=aabb, device=dev), o, d, t_min, sample_mode=mode, fused=f, **kw) for f in (True, False)]
    r64 = ref.march(aabb, o, d, t_min, radii.to(dev), None, step, kw["radius_scale_max"], mode, kw["interval_type"], lo, hi)
    assert r64["pack_infos"].tolist() == [[0, 1], [1, 6]] and r64["pidx"][0].item() == 5      # shell 4 (r = 2) lost, shell 5 kept
    for out in outs:
        for f in FIELDS_INT:
            assert torch.equal(getattr(out, f), r64[f]), f
        assert torch.isfinite(out.samples).all() and torch.isfinite(out.deltas).all()
    torch.testing.assert_close(outs[0].samples, outs[1].samples)
    torch.testing.assert_close(outs[0].depth_samples, outs[1].depth_samples)


def test_two_runs_give_the_same_bytes(dev):
    case = _case(67, SEEDS[67], "mixed")
    for mode, interval in (("box", "inverse_proportional"), ("spherical", "logarithm")):
        a, _ = _march(dev, case, mode, interval, 33, True, True, True)
        b, _ = _march(dev, case, mode, interval, 33, True, True, True)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def test_every_shell_valid_from_inside(dev):
    case = _case(67, SEED_INSIDE, "inside")
    for mode in ref.MODES:
        fused, _ = _march(dev, case, mode, "inverse_proportional", 33, True, False, True)
        n = ref.shell_table(R_MIN, R_MAX, 33, "inverse_proportional")[0].numel()
        assert fused.ridx_hit.tolist() == list(range(67)) and (fused.pack_infos[:, 1] == n).all()
        assert fused.samples.shape == (67 * n, 4) and torch.isfinite(fused.samples).all() and torch.isfinite(fused.deltas).all()
        assert (fused.samples[:, :3].norm(dim=-1) < 1.7321).all()
        if mode in ("box", "ellipsoid"):                       # radius = norm: 1 / r in [0, 1] maps into [-1, 1]
            assert (fused.samples[:, 3].abs() <= 1).all()


def test_binding_checks(dev):
    from nr3d_lib_amd.bindings import _nerfpp_march
    aabb, o, d, t_min = _case(5, SEEDS[5], "mixed")
    radii = ref.shell_table(R_MIN, R_MAX, 8, "inverse_proportional", device=dev)[0]
    ok = dict(last_radius=R_MAX)
    assert _nerfpp_march.nerfpp_march(o, d, t_min, aabb, radii, **ok) is not None
    for bad, what in (((o.double(), d, t_min, aabb, radii), "float32"), ((o, d[:, :2].contiguous(), t_min, aabb, radii), "rays_d"),
                      ((o, d, t_min[:3], aabb, radii), "t_min"), ((o, d, t_min, aabb.view(6), radii), "aabb"),
                      ((o, d, t_min, aabb, radii.view(2, 4)), "radii"), ((o.t().contiguous().t(), d, t_min, aabb, radii), "contiguous"),
                      ((o, d, t_min, aabb, radii, torch.rand(5, 7, device=dev)), "noise")):
        with pytest.raises(RuntimeError, match=what):
            _nerfpp_march.nerfpp_march(*bad, **ok)
