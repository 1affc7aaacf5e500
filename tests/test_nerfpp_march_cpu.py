"""No GPU: the NeRF++ shell marcher's ABI and binding refusals, the project's torch chain and the float32 restatement of
tests/nerfpp_march_ref.py against the recording of the reference's own sampler (tests/golden/ref_nerfpp_march.npz: four sample modes x
three interval types x max_steps 8, 33, 100 on 12 rays), the shell count, the refused modes, the input condition of every ray set the
GPU tests use, and the fall-back of the fused switch."""
import functools
import importlib
import os
import types

import numpy as np
import pytest
import torch

import nerfpp_march_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_nerfpp_march.npz")
FIELDS = ("ridx_hit", "samples", "depth_samples", "deltas", "ridx", "pack_infos")
STEPS = (8, 33, 100)
CASES = [(m, i, s) for m in ref.MODES for i in ref.INTERVALS for s in STEPS]


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def _space(aabb):
    from nr3d_lib_amd.models.spatial import AABBSpace
    return AABBSpace(aabb=aabb)


def _same(got, key, what):
    g = _golden()
    if key + ".none" in g:
        assert all(getattr(got, f) is None for f in FIELDS) if not isinstance(got, dict) else got is None, f"{what} {key}"
        return
    for f in FIELDS:
        want = torch.from_numpy(g[f"{key}.{f}"])
        have = got[f] if isinstance(got, dict) else getattr(got, f)
        if want.dtype == torch.int64:
            assert have.dtype == torch.int64 and torch.equal(have, want), f"{what} {key} {f}"
        else:
            torch.testing.assert_close(have, want, equal_nan=True, msg=lambda m: f"{what} {key} {f}: {m}")


def test_abi():
    from nr3d_lib_amd import _abi
    assert _abi.ABI_VERSION >= 26
    head = ['uint32_t', 'ptr', 'ptr', 'ptr', 'ptr', 'uint32_t', 'ptr', 'ptr', 'float', 'float', 'int', 'int', 'float', 'float']
    assert _abi.SIGNATURES['nr3d_nerfpp_march_count'] == ('int', head + ['ptr', 'ptr'])
    assert _abi.SIGNATURES['nr3d_nerfpp_march_emit'] == ('int', head + ['ptr', 'uint64_t', 'ptr', 'ptr', 'ptr', 'ptr', 'ptr'])


def test_binding_refuses_cpu_and_meta_tensors():
    from nr3d_lib_amd.bindings import _nerfpp_march
    aabb, o, d, t_min = ref.golden_rays()
    radii = ref.shell_table(1.0, 100.0, 8, "inverse_proportional")[0]
    with pytest.raises(RuntimeError, match="GPU only"):
        _nerfpp_march.nerfpp_march(o, d, t_min, aabb, radii, last_radius=100.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        _nerfpp_march.nerfpp_march(*(t.to("meta") for t in (o, d, t_min, aabb, radii)), last_radius=100.0)
    with pytest.raises(RuntimeError, match="sample_mode"):
        _nerfpp_march.nerfpp_march(o, d, t_min, aabb, radii, last_radius=100.0, sample_mode="lindisp")


@pytest.mark.parametrize("mode,interval,steps", CASES)
def test_chain_equals_the_recording(mode, interval, steps):
    from nr3d_lib_amd.graphics.raymarch import nerfpp_raymarch
    aabb, o, d, t_min = ref.golden_rays()
    got = nerfpp_raymarch(_space(aabb), o, d, t_min, None, radius_scale_min=1.0, radius_scale_max=100.0, include_inf_distance=True,
                          max_steps=steps, sample_mode=mode, interval_type=interval)
    _same(got, f"{mode}.{interval}.{steps}", "chain")


@pytest.mark.parametrize("mode,interval,steps", CASES)
def test_restatement_equals_the_recording(mode, interval, steps):
    aabb, o, d, t_min = ref.golden_rays()
    radii, step, lo, hi = ref.shell_table(1.0, 100.0, steps, interval)
    got = ref.march(aabb, o, d, t_min, radii, None, step, ref.last_radius(100.0, True), mode, interval, lo, hi, dtype=torch.float32)
    _same(got, f"{mode}.{interval}.{steps}", "restatement")


def test_the_recording_has_packs_of_every_kind():
    g = _golden()
    lens = set()
    for m, i, s in CASES:
        n = np.zeros(12, np.int64)
        n[g[f"{m}.{i}.{s}.ridx_hit"]] = g[f"{m}.{i}.{s}.pack_infos"][:, 1]
        lens |= set(n.tolist())
        assert not np.isnan(g[f"{m}.{i}.{s}.deltas"]).any()
    assert 0 in lens and 1 in lens and 101 in lens and any(1 < v < 8 for v in lens)


def test_shell_count_is_aranges_not_max_steps():
    from nr3d_lib_amd.graphics.raymarch import nerfpp_raymarch
    aabb, o, d, t_min = ref.golden_rays()
    assert ref.shell_table(1.0, 100.0, 100, "inverse_proportional")[0].numel() == 101
    assert ref.shell_table(1.0, 100.0, 100, "logarithm")[0].numel() == 100
    for interval, n in (("inverse_proportional", 101), ("logarithm", 100)):
        got = nerfpp_raymarch(_space(aabb), o[:1], d[:1], t_min[:1], radius_scale_min=1.0, radius_scale_max=100.0, max_steps=100,
                              interval_type=interval)
        assert got.pack_infos.tolist() == [[0, n]] and got.samples.shape == (n, 4)


@pytest.mark.parametrize("fused", [None, False, True])
def test_refused_modes(fused):
    from nr3d_lib_amd.graphics.raymarch import nerfpp_raymarch
    aabb, o, d, t_min = ref.golden_rays()
    space = _space(aabb)
    for mode in ("lindisp", "moving_spherical_shells"):
        with pytest.raises(RuntimeError, match="UnboundLocalError"):
            nerfpp_raymarch(space, o, d, t_min, sample_mode=mode, fused=fused)
    for mode in ("moving_far_spherical", "neurecon01", "neurecon02"):
        with pytest.raises(RuntimeError, match="no longer supported"):
            nerfpp_raymarch(space, o, d, t_min, sample_mode=mode, fused=fused)
    with pytest.raises(RuntimeError, match="Invalid sample_mode"):
        nerfpp_raymarch(space, o, d, t_min, sample_mode="shells", fused=fused)
    with pytest.raises(RuntimeError, match="Invalid interval_type"):
        nerfpp_raymarch(space, o, d, t_min, interval_type="linear", fused=fused)
    with pytest.raises(NotImplementedError):
        nerfpp_raymarch(types.SimpleNamespace(aabb=aabb), o, d, t_min, fused=fused)


def test_long_mode_names_are_aliases():
    from nr3d_lib_amd.graphics.raymarch import nerfpp_raymarch
    aabb, o, d, t_min = ref.golden_rays()
    for long, short in (("fixed_cuboid_shells", "box"), ("fixed_ellipsoid_shells", "ellipsoid"), ("fixed_cubic_shells", "cube"),
                        ("fixed_spherical_shells", "spherical")):
        a = nerfpp_raymarch(_space(aabb), o, d, t_min, max_steps=8, sample_mode=long, include_inf_distance=True)
        b = nerfpp_raymarch(_space(aabb), o, d, t_min, max_steps=8, sample_mode=short, include_inf_distance=True)
        for f in FIELDS:
            assert torch.equal(getattr(a, f), getattr(b, f))


def test_every_gpu_ray_set_is_clear_of_ties():
    """the input condition of tests/test_nerfpp_march_gpu.py and tests/test_nerf_distant_query_gpu.py, on the un-perturbed tables (the GPU
    tests assert it again on the noise they draw)"""
    import test_nerfpp_march_gpu as gpu_cases
    sets = gpu_cases.all_ray_sets()
    assert {ref.shell_table(gpu_cases.R_MIN, gpu_cases.R_MAX, s[4], s[3])[0].numel() for s in sets} >= set(gpu_cases.TABLE_LENGTHS)
    for R, seed, kind, interval, steps, inf in sets:
        aabb, o, d, t_min = ref.rays(R, seed, kind)
        radii, step, lo, hi = ref.shell_table(gpu_cases.R_MIN, gpu_cases.R_MAX, steps, interval)
        for mode in ref.MODES:
            n = ref.near_ties(aabb, o, d, t_min, radii, None, step, ref.last_radius(gpu_cases.R_MAX, inf), mode, interval)
            assert n == 0, f"R {R} seed {seed} {kind} steps {steps} {mode} {interval}: {n} near ties"


def test_near_ties_sees_a_tie():
    aabb, o, d, _ = ref.golden_rays()
    radii, step, lo, hi = ref.shell_table(1.0, 100.0, 8, "inverse_proportional")
    t = ref.march(aabb, o[:1], d[:1], torch.zeros(1), radii, None, step, 100.0, "box", "inverse_proportional", lo, hi)["depth_samples"]
    t_min = (t[3] * (1 + 5e-5)).float().view(1)
    assert ref.near_ties(aabb, o[:1], d[:1], t_min, radii, None, step, 100.0, "box", "inverse_proportional") >= 1
    assert ref.near_ties(aabb, o[:1], d[:1], torch.zeros(1), radii, None, step, 100.0, "box", "inverse_proportional") == 0


def test_switch_on_cpu_tensors_and_rays_with_grad_take_the_chain(monkeypatch):
    from nr3d_lib_amd.bindings import _nerfpp_march
    from nr3d_lib_amd.graphics.raymarch import nerfpp_raymarch as fn
    mod = importlib.import_module("nr3d_lib_amd.graphics.raymarch.nerfpp_raymarch")     # the function shadows the module in its package

    def boom(*a, **k):
        raise AssertionError("the fused route was taken")

    monkeypatch.setattr(_nerfpp_march, "nerfpp_march", boom)
    monkeypatch.setattr(mod, "FUSED_NERFPP_MARCH", True)
    aabb, o, d, t_min = ref.golden_rays()
    a = fn(_space(aabb), o, d, t_min, max_steps=8)
    b = fn(_space(aabb), o, d, t_min, max_steps=8, fused=True)
    c = fn(_space(aabb), o, d, t_min, max_steps=8, fused=False)
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(c, f)) and torch.equal(getattr(b, f), getattr(c, f))
    o_g = o[:7].clone().requires_grad_(True)                   # the rays without a zero direction component (its slabs are infinite)
    g = fn(_space(aabb), o_g, d[:7], t_min[:7], max_steps=8, fused=True)
    assert g.samples.requires_grad
    g.samples.sum().backward()
    assert o_g.grad is not None and torch.isfinite(o_g.grad).all()


def test_mixin_delegates():
    from nr3d_lib_amd.models.fields_distant.nerf import NeRFRendererMixinDistant

    class Net:
        def __init__(self, aabb=None):
            self.space = _space(aabb)

    class Model(NeRFRendererMixinDistant, Net):
        pass

    aabb, o, d, t_min = ref.golden_rays()
    m = Model(radius_scale_max=100.0, include_inf_distance=True, aabb=aabb)
    got = m._ray_marching(o, d, t_min, None, max_steps=33, sample_mode="cube", interval_type="logarithm")
    _same(got, "cube.logarithm.33", "mixin")
    with pytest.raises(AssertionError):
        NeRFRendererMixinDistant()
    with pytest.raises(NotImplementedError):
        m.ray_test(o, d)
