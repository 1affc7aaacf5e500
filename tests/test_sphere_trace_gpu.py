"""GPU: csrc/sphere_trace.hip through bindings._sphere_trace against the numpy restatement (tests/sphere_trace_ref.py).  Every
comparison is bit-exact and over ALL rays: both sides make the same float32 decisions, ties included, and the distances both sides
consume are the same float32 array (evaluated once on the host from the GPU's own query positions)."""
import numpy as np
import pytest
import torch

import sphere_trace_ref as R
from sphere_trace_ref import sphere_sdf

pytestmark = pytest.mark.gpu
F = np.float32


def B():
    from nr3d_lib_amd.bindings import _sphere_trace
    return _sphere_trace


def same(got, want, what):
    """bit-exact: same shape, dtype and bytes"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint8).reshape(got.shape[0], -1) != want.view(np.uint8).reshape(want.shape[0], -1)).any(1))[0]
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} rows differ, first {bad[:5]}: got {got[bad[:3]]}, want {want[bad[:3]]}")


def to(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def ray_set(rng, n_side=20):
    """pinhole camera inside the grid, rays starting anywhere inside, axis-parallel rays (zero components, both signs), rays that miss
    (starting outside the grid, or pointing away from it)"""
    u = np.linspace(-0.8, 0.8, n_side)
    U, V = np.meshgrid(u, u, indexing="ij")
    d_cam = np.stack([U.ravel(), V.ravel(), np.ones(U.size)], -1)
    o_cam = np.tile(np.array([0.1, -0.2, -0.93]), (d_cam.shape[0], 1))
    m = 300
    o_in = rng.uniform(-0.99, 0.99, (m, 3))
    d_in = rng.standard_normal((m, 3))
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    o_ax = rng.uniform(-0.9, 0.9, (60, 3))
    d_ax = axes[np.arange(60) % 6]
    o_ax[:6] = np.round(o_ax[:6] * 4) / 4               # starts exactly on voxel boundaries as well
    o_out = rng.uniform(1.5, 3.0, (60, 3)) * rng.choice([-1, 1], (60, 3))
    d_out = rng.standard_normal((60, 3))
    d_out[:30] = -o_out[:30]                            # aimed at the grid from outside
    o = np.concatenate([o_cam, o_in, o_ax, o_out])
    d = np.concatenate([d_cam, d_in, d_ax, d_out])
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    n = o.shape[0]
    near = np.where(np.arange(n) % 3 == 0, 0.05, 0.0)
    far = rng.uniform(0.3, 4.0, n)
    return o.astype(F), d.astype(F), near.astype(F), far.astype(F)


def make_grid(kind, rng):
    if kind == "random32":
        return rng.random((32, 32, 32)) < 0.5
    if kind == "random128":
        return rng.random((128, 128, 128)) < 0.5
    if kind == "shell64":
        c = (np.arange(64) + 0.5) / 64 * 2 - 1
        X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
        g = np.abs(np.sqrt(X * X + Y * Y + Z * Z) - 0.6) < 0.022
        assert 0.02 <= g.mean() <= 0.03, g.mean()
        return g
    if kind == "empty":
        return np.zeros((16, 16, 16), bool)
    if kind == "full":
        return np.ones((16, 16, 16), bool)
    assert kind == "noncubic"
    return rng.random((16, 32, 8)) < 0.5


@pytest.mark.parametrize("kind", ["random32", "random128", "shell64", "empty", "full", "noncubic"])
def test_ray_march_matches_restatement(dev, kind):
    rng = np.random.default_rng(7)
    grid = make_grid(kind, rng)
    o, d, near, far = ray_set(rng)
    want = R.ray_march(grid, o, d, near, far, return_pts=True)
    g = B().DenseGrid(*grid.shape, to(dev, grid)[0])
    assert g.res == grid.shape
    for return_pts in (False, True):
        valid, pack, segs, pts, dbg = B().ray_march(g, *to(dev, o, d, near, far), return_pts=return_pts)
        assert dbg == {}
        same(valid, want[0], f"{kind} valid_rays_idx")
        same(pack, want[1], f"{kind} segs_pack_info")
        same(segs, want[2], f"{kind} segs")
        if return_pts:
            same(pts, want[3], f"{kind} segs_endpoints")
        else:
            assert pts is None
    if kind == "empty":
        assert valid.numel() == 0 and segs.shape == (0, 2)
    else:
        assert valid.numel() > 100


ALIVE_KEYS = ("pos", "dir", "idx", "t", "n_steps", "status", "debug_flag", "hit_region_infos", "hit_seg_regions", "seg_idxs", "seg_end_idxs")
HIT_KEYS = ("pos", "dir", "idx", "t", "n_steps")


def compare_state(tr, ref, what):
    a, h = tr.get_rays(B().ALIVE), tr.get_rays(B().HIT)
    ra, rh = ref.get_rays(R.ALIVE), ref.get_rays(R.HIT)
    assert int(a["n_rays"]) == tr.n_rays(B().ALIVE) == ref.n_alive and int(h["n_rays"]) == tr.n_rays(B().HIT) == ref.n_rays(R.HIT), what
    assert tr.n_rays(B().OUT) == ref.n_rays(R.OUT)
    for k in ALIVE_KEYS:
        same(a[k], ra[k], f"{what}: alive {k}")
    for k in HIT_KEYS:
        same(h[k], rh[k], f"{what}: hit {k}")
    same(tr.get_trace_positions(), ref.positions(), f"{what}: trace positions")


def sphere_case(dev, min_step=0.01, thr=1e-3, scale=1.0, zero_offset=0.0):
    grid, o, d, near, far = R.sphere_scene()
    valid, pack, segs, _ = R.ray_march(grid, o, d, near, far)
    tr = B().SphereTracer(min_step, scale, zero_offset, thr)
    ref = R.SphereTracer(min_step, scale, zero_offset, thr)
    dv = to(dev, o, d, valid, pack, segs)
    tr.init_rays(*dv)
    ref.init_rays(o, d, valid, pack, segs)
    return tr, ref, dv


def step_both(tr, ref, sdf=sphere_sdf, spoil=None):
    """one advance of both sides from the same float32 distances, evaluated once on the host at the GPU's positions"""
    x = tr.get_trace_positions().cpu().numpy()
    dist = sdf(x)
    if spoil is not None:
        dist = spoil(dist)
    tr.advance_rays(torch.from_numpy(dist).to(tr._dev))
    ref.advance_rays(dist)


@pytest.mark.parametrize("scale,zero_offset", [(1.0, 0.0), (1.6, 0.013)])
def test_tracer_step_by_step(dev, scale, zero_offset):
    tr, ref, _ = sphere_case(dev, scale=scale, zero_offset=zero_offset)
    compare_state(tr, ref, "init")
    i, seen_back, seen_interp = 1, False, False
    while i < 400 and ref.n_alive > 0:
        for _ in range(min(i, 4)):
            step_both(tr, ref)
            compare_state(tr, ref, f"advance {i}")
            seen_back |= bool((ref.dbg == -1).any())
            seen_interp |= bool((ref.dbg == 126).any())
            i += 1
        assert tr.compact_rays() == ref.compact_rays()
        compare_state(tr, ref, f"compact {i}")
    assert ref.n_alive == 0 and ref.n_rays(R.HIT) > 100 and ref.n_rays(R.OUT) > 10
    if scale == 1.0:
        return
    assert seen_back      # an over-estimating distance (zero_offset) makes rays step back, so that branch is compared too


def torch_sphere(x):
    return torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]) - 0.5


def full_trace(dev, between, iters=1000):
    grid, o, d, near, far = R.sphere_scene()
    g = B().DenseGrid(*grid.shape, to(dev, grid)[0])
    od = to(dev, o, d, near, far)
    valid, pack, segs, _, _ = B().ray_march(g, *od)
    tr = B().SphereTracer(0.01, 1.0)
    tr.trace(od[0], od[1], torch_sphere, between, iters, valid, pack, segs)
    return tr, valid, pack, segs


def test_two_traces_are_byte_identical(dev):
    outs = []
    for _ in range(2):
        tr, valid, pack, segs = full_trace(dev, 4)
        h = tr.get_rays(B().HIT)
        outs.append([valid, pack, segs] + [h[k] for k in HIT_KEYS])
        assert tr.n_rays(B().ALIVE) == 0 and h["idx"].numel() > 100
    for a, b in zip(*outs):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_compaction_cadence_does_not_change_a_ray(dev):
    res = []
    for between in (1, 4):
        tr, valid, _, _ = full_trace(dev, between, iters=5000)
        assert tr.n_rays(B().ALIVE) == 0
        h = tr.get_rays(B().HIT)
        order = torch.argsort(h["idx"])
        res.append((h["idx"][order].cpu().numpy(), h["t"][order].cpu().numpy(), h["n_steps"][order].cpu().numpy(), tr.n_rays(B().OUT)))
    for a, b in zip(*res):          # the same rays hit (so the same are OUT), at the same t after the same number of steps
        assert np.array_equal(a, b)


def test_bad_distances_end_their_rays_only(dev):
    tr, ref, _ = sphere_case(dev)
    for _ in range(2):
        step_both(tr, ref)
    assert tr.compact_rays() == ref.compact_rays()
    n = ref.n_alive
    assert n > 200
    bad = {3: np.nan, 10: np.inf, 17: -np.inf, 40: -1e30, 41: 1e30, n - 1: np.nan, 0: -1e30}
    idx_bad = ref.idx[[k for k, v in bad.items() if not np.isfinite(v)]].copy()

    def spoil(dist):
        dist = dist.copy()
        for k, v in bad.items():
            dist[k] = v
        return dist

    step_both(tr, ref, spoil=spoil)
    compare_state(tr, ref, "spoiled advance")
    st = tr.get_rays(B().ALIVE)["status"].cpu().numpy()
    assert all(st[k] == R.OUT for k, v in bad.items() if not np.isfinite(v))
    for j in range(6):              # +-1e30 are finite: those rays go on (bounded steps), everything stays comparable
        step_both(tr, ref, spoil=spoil if j == 2 else None)
        compare_state(tr, ref, f"after spoiled {j}")
        if j % 2:
            assert tr.compact_rays() == ref.compact_rays()
            compare_state(tr, ref, f"compact after spoiled {j}")
            bad = {k: v for k, v in bad.items() if k < ref.n_alive}
    torch.cuda.synchronize()
    alive_or_hit = np.concatenate([ref.idx, ref.hits[0]])
    assert not np.isin(idx_bad, alive_or_hit).any()


def test_tail_sampling(dev):
    tr, ref, _ = sphere_case(dev, min_step=0.05)
    for i in range(3):
        step_both(tr, ref)
    assert tr.compact_rays() == ref.compact_rays() > 50
    step = 0.02
    got = tr.sample_on_segments(step)
    want = ref.sample_on_segments(step)
    for g, w, name in zip(got, want, ("offsets", "counts", "depths", "positions")):
        same(g, w, f"sample_on_segments {name}")
    assert got[2].numel() > 500
    dist = sphere_sdf(got[3].cpu().numpy())
    n_hit0 = tr.n_rays(B().HIT)
    tr.trace_on_samples(got[0], got[1], got[2], torch.from_numpy(dist).to(dev))
    ref.trace_on_samples(*want[:3], dist)
    assert tr.n_rays(B().HIT) > n_hit0
    compare_state(tr, ref, "trace_on_samples")


def test_empty_inputs_everywhere(dev):
    b = B()
    g = b.DenseGrid(4, 4, 4, torch.ones(4, 4, 4, dtype=torch.bool, device=dev))
    e3, e1 = torch.empty((0, 3), device=dev), torch.empty(0, device=dev)
    valid, pack, segs, pts, _ = b.ray_march(g, e3, e3, e1, e1, return_pts=True)
    assert valid.shape == (0,) and valid.dtype == torch.int64 and pack.shape == (0, 2) and pack.dtype == torch.int32
    assert segs.shape == (0, 2) and pts.shape == (0, 2, 3)
    # rays, but none valid (empty grid), then a tracer over zero valid rays
    ge = b.DenseGrid(4, 4, 4, torch.zeros(4, 4, 4, dtype=torch.bool, device=dev))
    o, d = torch.zeros((5, 3), device=dev), torch.tensor([[0., 0., 1.]], device=dev).repeat(5, 1)
    valid, pack, segs, pts, _ = b.ray_march(ge, o, d, torch.zeros(5, device=dev), torch.ones(5, device=dev))
    assert valid.numel() == 0 and segs.shape == (0, 2) and pts is None
    for ro, rd in ((e3, e3), (o, d)):
        tr = b.SphereTracer(0.1, 1.0)
        calls = []
        tr.trace(ro, rd, lambda x: calls.append(1) or x[:, 0], 4, 100, valid, pack, segs)
        assert not calls and tr.compact_rays() == 0 and tr.get_trace_positions().shape == (0, 3)
        tr.advance_rays(e1)
        for s in (b.ALIVE, b.HIT):
            r = tr.get_rays(s)
            assert int(r["n_rays"]) == 0 and r["pos"].shape == (0, 3) and r["idx"].dtype == torch.int64 and r["n_steps"].dtype == torch.int32
        assert tr.get_rays(b.ALIVE)["status"].dtype == torch.uint8 and tr.get_rays(b.ALIVE)["debug_flag"].dtype == torch.int8
        s = tr.sample_on_segments(0.1)
        assert [t.shape for t in s] == [(0,), (0,), (0,), (0, 3)] and s[0].dtype == torch.int32
        tr.trace_on_samples(s[0], s[1], s[2], e1)
        assert tr.n_rays(b.HIT) == 0 and tr.n_rays(b.OUT) == 0
    # all rays finished: zero ALIVE rays with a non-empty history
    tr, _, _, _ = full_trace(dev, 4)
    assert tr.n_rays(b.ALIVE) == 0 and tr.compact_rays() == 0 and tr.get_trace_positions().shape == (0, 3)
    tr.advance_rays(e1)
    assert tr.sample_on_segments(0.1)[2].numel() == 0


def test_argument_errors_name_the_argument(dev):
    b = B()
    g = b.DenseGrid(4, 4, 4, torch.ones(4, 4, 4, dtype=torch.bool, device=dev))
    o, d = torch.zeros((5, 3), device=dev), torch.ones((5, 3), device=dev)
    n, f = torch.zeros(5, device=dev), torch.ones(5, device=dev)
    with pytest.raises(RuntimeError, match="grid_occ"):
        b.DenseGrid(4, 4, 8, torch.ones(4, 4, 4, dtype=torch.bool, device=dev))
    with pytest.raises(RuntimeError, match="grid_occ"):
        b.DenseGrid(4, 4, 4, torch.ones(4, 4, 4, device=dev))
    with pytest.raises(RuntimeError, match="rays_d"):
        b.ray_march(g, o, d[:4], n, f)
    with pytest.raises(RuntimeError, match="rays_o"):
        b.ray_march(g, o.double(), d, n, f)
    with pytest.raises(RuntimeError, match="rays_far"):
        b.ray_march(g, o, d, n, f[:3])
    with pytest.raises(RuntimeError, match="rays_o.*contiguous"):
        b.ray_march(g, torch.zeros((3, 5), device=dev).t(), d, n, f)
    with pytest.raises(RuntimeError, match="enable_debug"):
        b.ray_march(g, o, d, n, f, enable_debug=True)
    valid, pack, segs, _, _ = b.ray_march(g, o, d, n, f)
    tr = b.SphereTracer(0.1, 1.0)
    with pytest.raises(RuntimeError, match="segs_endpoint_distances"):
        tr.init_rays(o, d, valid, pack, segs, segs)
    with pytest.raises(RuntimeError, match="segs_pack_info"):
        tr.init_rays(o, d, valid, pack.long(), segs)
    tr.init_rays(o, d, valid, pack, segs)
    with pytest.raises(RuntimeError, match="distances"):
        tr.advance_rays(torch.zeros(valid.numel() + 1, device=dev))
    with pytest.raises(ValueError, match="OUT"):
        tr.get_rays(b.OUT)
    with pytest.raises(RuntimeError, match="step_size"):
        tr.sample_on_segments(0.0)


def torus_sdf_np(x, R0=0.5, r0=0.2):
    x = x.astype(np.float64)
    q = np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) - R0
    return np.sqrt(q * q + x[..., 2] ** 2) - r0


def torus_sdf_torch(x):
    q = torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) - 0.5
    return torch.sqrt(q * q + x[:, 2] * x[:, 2]) - 0.2


@pytest.mark.parametrize("shape", ["sphere", "torus"])
def test_graphics_tracer_hits_the_analytic_set(dev, shape):
    """graphics.sphere_trace.SphereTracer.trace with the SDF as a torch function.  The fan keeps only rays whose closest approach
    clears tangency: min over the ray of the exact SDF (float64, sampled every 1e-3 of ray length, so known to 1e-3 as an SDF is
    1-Lipschitz) is beyond 4e-3 on either side, i.e. the true value beyond 3e-3 > 2 * hit_threshold.  The restatement traced on the CPU
    confirms that no ray of that fan is left out; hit points lie on the surface to the bound derived in test_sphere_trace_cpu.py."""
    from nr3d_lib_amd.graphics.sphere_trace import DenseGrid, SphereTracer
    min_step, thr = 0.01, 1e-3
    sdf_np = (lambda x: sphere_sdf(x).astype(np.float64)) if shape == "sphere" else torus_sdf_np
    sdf_t = torch_sphere if shape == "sphere" else torus_sdf_torch
    res = 32
    c = (np.arange(res) + 0.5) / res * 2 - 1
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    grid = sdf_np(np.stack([X, Y, Z], -1)) < 2 * np.sqrt(3) / res
    u = np.linspace(-0.75, 0.75, 28)
    U, V = np.meshgrid(u, u, indexing="ij")
    d = np.stack([U.ravel() + 0.3, V.ravel() - 0.2, np.ones(U.size)], -1)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    o = np.tile(np.array([-0.2, 0.15, -0.95], F), (d.shape[0], 1))
    ts = np.arange(0, 3.5, 1e-3)
    closest = np.stack([sdf_np(o.astype(np.float64) + t * d.astype(np.float64)) for t in ts], 0).min(0)
    keep = np.abs(closest) > 4e-3
    o, d, closest = o[keep], d[keep], closest[keep]
    assert keep.mean() > 0.9 and np.abs(closest).min() > 2 * thr
    analytic = closest < 0
    assert analytic.sum() > 100 and (~analytic).sum() > 100
    near, far = np.zeros(o.shape[0], F), np.full(o.shape[0], 3.5, F)
    # the restatement on the CPU: the chosen fan leaves no ray out
    valid, pack, segs, _ = R.ray_march(grid, o, d, near, far)
    ref = R.SphereTracer(min_step, 1.0, 0.0, thr)
    ref.trace(o, d, lambda x: sdf_np(x).astype(F), 4, 1000, valid, pack, segs)
    ref_hit = np.zeros(o.shape[0], bool)
    ref_hit[ref.get_rays(R.HIT)["idx"]] = True
    assert np.array_equal(ref_hit, analytic)
    # the GPU
    to_, td, tn, tf = to(dev, o, d, near, far)
    tracer = SphereTracer(DenseGrid(res, res, res, to(dev, grid)[0]), min_step=min_step, hit_threshold=thr)
    out = tracer.trace(dict(rays_o=to_, rays_d=td, near=tn, far=tf), lambda x: dict(sdf=sdf_t(x)))
    got = np.zeros(o.shape[0], bool)
    idx = out["idx"].cpu().numpy()
    got[idx] = True
    assert idx.shape[0] == np.unique(idx).shape[0] and np.array_equal(got, analytic)
    err = np.abs(sdf_np(out["pos"].cpu().numpy()))
    assert err.max() <= max(2 * thr, 1.1 * min_step), err.max()
    assert tracer.last_march_iters > 0 and tracer.backend.n_rays(B().ALIVE) == 0
    # tail sampling finishes what a short march leaves: same hit set
    tail = SphereTracer(DenseGrid(res, res, res, to(dev, grid)[0]), min_step=min_step, hit_threshold=thr, max_march_iters=6,
                        tail_sample_threshold=1, tail_sample_step_size=0.004)
    out2 = tail.trace(dict(rays_o=to_, rays_d=td, near=tn, far=tf), sdf_t)
    assert tail.last_march_iters == 7            # compaction cadence 1, 2, 4: the first check of max_march_iters = 6 that fails
    assert np.array_equal(np.sort(out2["idx"].cpu().numpy()), np.sort(idx))
    err2 = np.abs(sdf_np(out2["pos"].cpu().numpy()))
    assert err2.max() <= max(2 * thr, 1.1 * min_step, 0.004), err2.max()


class _Occ:
    def __init__(self, grid):
        self.resolution = torch.tensor(grid.shape)
        self.occ_grid = grid


class _Accel:
    def __init__(self, grid):
        self.occ = _Occ(grid)


class _Model:
    def __init__(self, grid):
        self.accel = _Accel(grid)

    def forward_sdf(self, x, **kw):
        return dict(sdf=torch_sphere(x))

    def forward_inv_s(self):
        return torch.tensor(64.0)

    def forward(self, x, nablas_has_grad=False, with_rgb=True, with_normal=True, **kw):
        out = dict(sdf=torch_sphere(x))
        if with_normal:
            out["nablas"] = torch.nn.functional.normalize(x, dim=-1)
        if with_rgb:
            out["rgb"] = x.abs()
        return out


def test_neus_ray_query_sphere_trace(dev):
    from nr3d_lib_amd.graphics.neus import neus_ray_query_sphere_trace
    grid, o, d, near, far = R.sphere_scene()
    model = _Model(to(dev, grid)[0])
    to_, td, tn, tf = to(dev, o, d, near, far)
    n = o.shape[0]
    rays = dict(num_rays=n, rays_o=to_, rays_d=td, near=tn, far=tf, rays_inds=torch.arange(n, device=dev))
    buf, details = neus_ray_query_sphere_trace(model, rays, min_step=0.01)
    assert details == {'render.num_per_ray': 1} and buf["type"] == "batched" and buf["num_per_hit"] == 1
    assert set(buf) == {"type", "rays_inds_hit", "num_per_hit", "t", "opacity_alpha", "net_x", "nablas", "rgb"}
    assert buf["t"].shape == (n, 1) and buf["opacity_alpha"].shape == (n, 1) and buf["net_x"].shape == (n, 1, 3)
    assert buf["nablas"].shape == (n, 1, 3) and buf["rgb"].shape == (n, 1, 3)
    hit = model.tracer.backend.get_rays(B().HIT)
    must, must_not = R.analytic_sphere_hits(o, d, 0.5, 2e-3)
    alpha = buf["opacity_alpha"][:, 0].cpu().numpy()
    assert set(np.unique(alpha)) == {0.0, 1.0} and (alpha[must] == 1).all() and (alpha[must_not] == 0).all()
    assert np.array_equal(np.nonzero(alpha == 1)[0], np.sort(hit["idx"].cpu().numpy()))
    assert torch.equal(buf["net_x"][hit["idx"], 0], hit["pos"]) and float(buf["net_x"][torch.from_numpy(alpha == 0).to(dev)].abs().max()) == 0
    assert torch.equal(buf["rgb"][hit["idx"], 0], hit["pos"].abs())
    buf, details = neus_ray_query_sphere_trace(model, rays, with_rgb=False, with_normal=False, min_step=0.01)
    assert "net_x" not in buf and "rgb" not in buf and buf["opacity_alpha"].sum() == hit["idx"].numel()
    # zero rays, and rays that hit nothing: the (empty, {}) pair both times
    e3, e1 = torch.empty((0, 3), device=dev), torch.empty(0, device=dev)
    for r in (dict(num_rays=0, rays_o=e3, rays_d=e3, near=e1, far=e1, rays_inds=e1.long()),
              dict(num_rays=4, rays_o=to_[:4], rays_d=-td[:4], near=tn[:4], far=tf[:4], rays_inds=torch.arange(4, device=dev))):
        buf, details = neus_ray_query_sphere_trace(model, r)
        assert buf == dict(type="empty", rays_inds_hit=[]) and details == {}
