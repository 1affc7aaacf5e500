"""CPU: the sphere tracer's restatement (tests/sphere_trace_ref.py) pinned by hand-evaluated answers, a sphere traced by it, and the
boundary of the port (bindings._sphere_trace, the nr3d_sphere_trace_* symbols)."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import sphere_trace_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_fma32_is_correctly_rounded():
    """fma32 against exact rational arithmetic rounded once (cancellations and near-ties included)"""
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(F)
    b = rng.standard_normal(4000).astype(F)
    c = rng.standard_normal(4000).astype(F)
    c[:1000] = -(a[:1000] * b[:1000])                          # cancellation: the result is the product's rounding error
    c[1000:2000] = (a[1000:2000] * b[1000:2000]) * F(2.0 ** 24)     # the product lands near half an ulp of c
    got = R.fma32(a, b, c)

    def round32(q):
        if q == 0:
            return F(0)
        f = F(float(q))                                         # one candidate; walk to the nearest, ties to even
        best = f
        for cand in (np.nextafter(f, F(-np.inf)), np.nextafter(f, F(np.inf))):
            dc, db = abs(Fraction(float(cand)) - q), abs(Fraction(float(best)) - q)
            if dc < db or (dc == db and (int(cand.view(np.int32)) & 1) == 0):
                best = cand
        return best

    for i in range(a.shape[0]):
        want = round32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)


def _grid4():
    g = np.zeros((4, 4, 4), bool)
    g[1, 2, 2] = g[3, 2, 2] = g[2, 2, 1] = True
    return g


def test_ray_march_known_answers():
    """A 4^3 grid over [-1, 1]^3: a voxel is 0.5 wide, grid coordinates are (x + 1) * 2, a unit direction is 2 grid units long, so
    inv_dir = 1 / (2 + 1e-10f) = 0.5 exactly (and 1 / 1e-10f ~ 1e10 on the zero components: their boundary distances, 5e9, never win
    the first-minimum choice).  Occupied: (1,2,2), (3,2,2), (2,2,1).  Every number below is exact in float32.
      ray 0  o = (-1.5, .25, .25), d = +x, near .75: starts at grid (0.5, 2.5, 2.5) in empty voxel (0,2,2); enters voxel 1 at grid x = 1,
             t = (1 - (-1)) * 0.5 = 1.0; leaves at x = 2, t = 1.5; enters voxel 3 at x = 3, t = 2.0; leaves the grid at x = 4, t = 2.5:
             two separated runs (1.0, 1.5), (2.0, 2.5).
      ray 1  o = (.25, .25, .75), d = -z (signbit set: dir_sign 0, inv_dir -0.5): starts at grid z = 3.5 in (2,2,3), walks z = 3, 2 and
             enters (2,2,1) at grid z = 2: t = (2 - 3.5) * -0.5 = 0.75, leaves at z = 1: t = 1.25; (2,2,0) is empty, then outside.
      ray 2  o = (-.25, .25, .25), d = +x, near 0: starts INSIDE occupied (1,2,2) at grid x = 1.5: t_enter = (1.5 - 1.5) * 0.5 = 0, no walk
             first; leaves at x = 2: 0.25; second run from x = 3: 0.75 to x = 4: 1.25.
      ray 3  o = (-3, .25, .25), d = +x, near 0: the start (grid x = -4) is outside the grid; one step to voxel x = -3, still outside: no
             segment, although the line crosses both occupied voxels (the reference only marches from inside the grid).
      ray 4  ray 0 with far = 1.25, inside its first run: (1.0, min(1.5, 1.25)) and the march ends there."""
    o = np.array([[-1.5, .25, .25], [.25, .25, .75], [-.25, .25, .25], [-3, .25, .25], [-1.5, .25, .25]], F)
    d = np.array([[1, 0, 0], [0, 0, -1], [1, 0, 0], [1, 0, 0], [1, 0, 0]], F)
    near = np.array([.75, 0, 0, 0, .75], F)
    far = np.array([10, 10, 10, 10, 1.25], F)
    valid, pack, segs, pts = R.ray_march(_grid4(), o, d, near, far, return_pts=True)
    assert valid.tolist() == [0, 1, 2, 4]
    assert pack.tolist() == [[0, 2], [2, 1], [3, 2], [5, 1]] and pack.dtype == np.int32
    assert segs.tolist() == [[1.0, 1.5], [2.0, 2.5], [0.75, 1.25], [0.0, 0.25], [0.75, 1.25], [1.0, 1.25]]
    # endpoints o + d * t: ray 0's first segment runs from x = -0.5 to x = 0, ray 1's from z = 0 to z = -0.5
    assert pts[0].tolist() == [[-0.5, .25, .25], [0.0, .25, .25]] and pts[2].tolist() == [[.25, .25, 0.0], [.25, .25, -0.5]]
    # each case alone gives the same rows (nothing depends on the batch)
    for i, want in enumerate([[[1.0, 1.5], [2.0, 2.5]], [[0.75, 1.25]], [[0.0, 0.25], [0.75, 1.25]], [], [[1.0, 1.25]]]):
        v, p, s, _ = R.ray_march(_grid4(), o[i:i + 1], d[i:i + 1], near[i:i + 1], far[i:i + 1])
        assert s.tolist() == want and v.tolist() == ([0] if want else []) and p.tolist() == ([[0, len(want)]] if want else [])


def test_ray_march_empty_full_and_no_rays():
    o, d = np.array([[-.9, .1, .1]], F), np.array([[1, 0, 0]], F)
    near, far = np.zeros(1, F), np.full(1, 5, F)
    v, p, s, _ = R.ray_march(np.zeros((4, 4, 4), bool), o, d, near, far)
    assert v.shape == (0,) and p.shape == (0, 2) and s.shape == (0, 2)
    # full grid: one run from the start (t = 0) to the far face x = 1: t = 1.9f (o.x = -0.9f: (4 - (1 - 0.9f) * 2) * 0.5)
    v, p, s, _ = R.ray_march(np.ones((4, 4, 4), bool), o, d, near, far)
    assert v.tolist() == [0] and p.tolist() == [[0, 1]] and s[0, 0] == 0 and s[0, 1] == (F(4) - (F(-.9) + F(1)) * F(2)) * F(.5)
    v, p, s, pts = R.ray_march(np.ones((4, 4, 4), bool), np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, F), np.zeros(0, F), True)
    assert v.shape == (0,) and p.shape == (0, 2) and s.shape == (0, 2) and pts.shape == (0, 2, 3)


def test_advance_known_answers():
    """One ray, one segment (0, 4), min_step 0.1, hit_threshold 1e-3, by hand (sphere_tracer.cu:36-91):
      init: t = 0, region (-1, 4, -1, 1).  d = 1: d0 < 0 -> start (t0, d0) = (0, 1); forward min(1, (4 - 0) * 0.8) = 1 -> t = 1, flag 1.
      d = 0.5: d >= 0 -> start (1, 0.5); forward 0.5 -> t = 1.5.   d = -0.25: end (t1, d1) = (1.5, -0.25); not a hit (|d| > 1e-3,
      width 0.5 > 0.11); backward min(0.5 / 2, max(0.25, 0.1)) = 0.25 -> t = 1.25, flag -1.   d = 0: HIT by threshold, t += 0, flag 127."""
    tr = R.SphereTracer(0.1, 1.0)
    o, d = np.zeros((1, 3), F), np.array([[0, 0, 1]], F)
    tr.init_rays(o, d, np.array([0]), np.array([[0, 1]], np.int32), np.array([[0, 4]], F))
    assert tr.t.tolist() == [0.0] and tr.hr.tolist() == [[-1, 4, -1, 1]] and tr.hs.tolist() == [[0, 1]]
    tr.advance_rays(np.array([1.0], F))
    assert (tr.t[0], tr.dbg[0], tr.n_steps[0], tr.status[0]) == (1.0, 1, 1, R.ALIVE) and tr.hr.tolist() == [[0, 4, 1, 1]]
    tr.advance_rays(np.array([0.5], F))
    assert tr.t[0] == 1.5 and tr.hr.tolist() == [[1, 4, 0.5, 1]]
    tr.advance_rays(np.array([-0.25], F))
    assert (tr.t[0], tr.dbg[0], tr.n_steps[0]) == (1.25, -1, 3) and tr.hr.tolist() == [[1, 1.5, 0.5, -0.25]] and tr.hs.tolist() == [[0, 1]]
    assert tr.positions().tolist() == [[0, 0, 1.25]]
    tr.advance_rays(np.array([0.0], F))
    assert (tr.t[0], tr.dbg[0], tr.n_steps[0], tr.status[0]) == (1.25, 127, 3, R.HIT)
    assert tr.compact_rays() == 0 and tr.get_rays(R.HIT)["t"].tolist() == [1.25] and tr.n_rays(R.HIT) == 1
    # a bracket no wider than 1.1 * min_step is interpolated: region (1, 1.1, 0.5, -0.5) -> k = 0.5, t = 1 + 0.5 * (1.1f - 1)
    tr.init_rays(o, d, np.array([0]), np.array([[0, 1]], np.int32), np.array([[0, 4]], F))
    tr.hr[0] = [1, 4, 0.5, 1]
    tr.t[0] = F(1.1)
    tr.advance_rays(np.array([-0.5], F))
    assert tr.status[0] == R.HIT and tr.dbg[0] == 126 and tr.t[0] == R.fma32(F(.5), F(1.1) - F(1), F(1))
    # beyond the last segment: OUT at its end; a non-finite distance: OUT, state untouched
    tr.init_rays(o, d, np.array([0, 0]), np.array([[0, 2], [0, 2]], np.int32), np.array([[0, .5], [1, 1.25]], F))
    tr.t[:] = 1.2
    tr.seg_idx[:] = 1
    tr.advance_rays(np.array([3.0, np.nan], F))
    assert tr.status.tolist() == [R.OUT, R.OUT] and tr.dbg.tolist() == [-127, -128] and tr.t.tolist() == [1.25, F(1.2)]


def test_sphere_is_hit_within_the_bound():
    """Every ray that should hit does, and its hit point lies within max(2 * hit_threshold, 1.1 * min_step) of the surface.  Why that
    bound: a HIT by threshold has |d| <= hit_threshold at the query point and moves it by d ALONG THE RAY, not along the normal, so the
    new point is at most |d| + |d| from the surface; a HIT by bracket interpolates inside a bracket of ray length <= 1.1 * min_step whose
    ends have opposite signs, so the surface crosses the bracket and the point is at most its width away (an SDF is 1-Lipschitz)."""
    min_step, thr = 0.01, 1e-3
    grid, o, d, near, far = R.sphere_scene()
    valid, pack, segs, _ = R.ray_march(grid, o, d, near, far)
    tr = R.SphereTracer(min_step, 1.0, 0.0, thr)
    tr.trace(o, d, R.sphere_sdf, 4, 1000, valid, pack, segs)
    hit = tr.get_rays(R.HIT)
    must, must_not = R.analytic_sphere_hits(o, d, 0.5, 2 * thr)
    assert must.sum() > 100 and must_not.sum() > 100
    got = np.zeros(o.shape[0], bool)
    got[hit["idx"]] = True
    assert got[must].all() and not got[must_not].any()
    assert hit["idx"].shape[0] == np.unique(hit["idx"]).shape[0]
    err = np.abs(np.linalg.norm(hit["pos"].astype(np.float64), axis=1) - 0.5)
    assert err.max() <= max(2 * thr, 1.1 * min_step), err.max()
    assert tr.n_rays(R.ALIVE) == 0 and tr.n_rays(R.OUT) == valid.shape[0] - hit["idx"].shape[0]


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_binding_surface():
    """the names of entry.cu:14-47"""
    import inspect
    from nr3d_lib_amd.bindings import _sphere_trace as B
    assert (int(B.ALIVE), int(B.HIT), int(B.OUT)) == (0, 1, 2) and B.RayStatus.HIT == B.HIT
    for name in ("init_rays", "compact_rays", "advance_rays", "get_rays", "get_trace_positions", "sample_on_segments",
                 "trace_on_samples", "trace", "n_rays"):
        assert callable(getattr(B.SphereTracer, name)), name
    sig = inspect.signature(B.SphereTracer.__init__)
    assert list(sig.parameters)[1:] == ["min_step", "distance_scale", "zero_offset", "hit_threshold"]
    assert sig.parameters["zero_offset"].default == 0.0 and sig.parameters["hit_threshold"].default == 0.001
    assert list(inspect.signature(B.ray_march).parameters) == ["grid", "rays_o", "rays_d", "rays_near", "rays_far", "return_pts", "enable_debug"]
    assert list(inspect.signature(B.SphereTracer.trace).parameters)[1:] == [
        "rays_o", "rays_d", "distance_function", "max_steps_between_compact", "max_march_iters", "valid_rays_idx", "segs_pack_info",
        "segs", "segs_endpoint_distances"]
    assert hasattr(B.DenseGrid, "res")
    import nr3d_lib_amd.graphics.sphere_trace as G
    assert G.DenseGrid is B.DenseGrid and G.__all__ == ["SphereTracer", "DenseGrid"]
    d = inspect.signature(G.SphereTracer.__init__).parameters
    assert (d["min_step"].default, d["hit_threshold"].default, d["max_steps_between_compact"].default, d["max_march_iters"].default,
            d["tail_sample_threshold"].default) == (.1, 1e-3, 4, 1000, 0)
    from nr3d_lib_amd.graphics.neus import neus_ray_query
    assert "neus_ray_query_sphere_trace" in neus_ray_query.__all__
    # no GPU here: a CPU tensor is refused, by name or as such
    import torch
    with pytest.raises(RuntimeError, match="grid_occ|CPU tensor"):
        B.DenseGrid(4, 4, 4, torch.zeros(4, 4, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="init_rays first"):
        B.SphereTracer(0.1, 1.0).compact_rays()


def test_library_exports_the_sphere_trace_symbols(hiplib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nr3d_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nr3d_sphere_trace_[A-Za-z0-9_]+)\s*\(", header)))
    assert len(declared) >= 12, declared
    for need in ("march_count", "march_write", "init", "advance", "compact", "gather_hit", "gather_alive", "sample_count", "sample_write",
                 "trace_on_samples"):
        assert f"nr3d_sphere_trace_{need}" in declared
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "nr3d_lib_amd", "libnr3d_hip.so")], capture_output=True,
                        text=True).stdout
    exported = set(re.findall(r" T (nr3d_sphere_trace_[A-Za-z0-9_]+)", nm))
    assert exported == set(declared), exported ^ set(declared)
    from nr3d_lib_amd import _abi
    assert _abi.ABI_VERSION >= 14 and all(s in _abi.SIGNATURES for s in declared)
    assert hiplib.nr3d_sphere_trace_state_bytes(5) == 8 * 62 and hiplib.nr3d_sphere_trace_hits_bytes(5) == 8 * 12
