"""GPU: marching cubes in HIP (csrc/marching_cubes.hip through bindings._marching_cubes) against the numpy restatement of
tests/marching_cubes_ref.py -- ``torch.equal`` on vertices and faces, no tolerance: the specification fixes the order and every float32
operation -- and nr3d_lib_amd/graphics/trianglemesh.py on analytic SDFs: manifold, Euler characteristic, distance of the vertices to the
surface, orientation of the normals, sparse == dense, and the PLY file end to end."""
import functools
import math

import numpy as np
import pytest
import torch

import marching_cubes_ref as R

pytestmark = pytest.mark.gpu


def _row(n, nan=False):
    v = np.random.default_rng(10 + n).standard_normal((3, 3, n)).astype(np.float32)
    if nan:
        v[np.random.default_rng(11 + n).random(v.shape) < 0.1] = np.nan
    return v


VOLUMES = {
    "noise": lambda: (R.noise_volume(), 0.0),                                             # (9, 11, 72): z crosses a 64-lane chunk
    "noise_T": lambda: (np.ascontiguousarray(R.noise_volume().transpose(2, 1, 0)), 0.0),    # (72, 11, 9)
    "noise_T2": lambda: (np.ascontiguousarray(R.noise_volume().transpose(1, 2, 0)), 0.0),   # (11, 72, 9)
    "nan": lambda: (R.nan_volume(), 0.0),
    "nan_T": lambda: (np.ascontiguousarray(R.nan_volume().transpose(2, 0, 1)), 0.0),
    "open": lambda: (R.noise_volume(pad=False), 0.0),
    "level": lambda: (R.noise_volume(), 0.37),
    "exact": lambda: (R.exact_volume(), 0.0),
    "nz2": lambda: (np.ascontiguousarray(R.noise_volume()[:, :, 1:3]), 0.0),
    "nx2": lambda: (np.ascontiguousarray(R.noise_volume()[1:3]), 0.0),
    "ny2": lambda: (np.ascontiguousarray(R.noise_volume()[:, 1:3]), 0.0),
    "cell": lambda: (np.ascontiguousarray(R.noise_volume(pad=False)[:2, :2, :2]), 0.0),
    "outside": lambda: (np.ones((5, 6, 7), np.float32), 0.0),
    "inside": lambda: (-np.ones((5, 6, 7), np.float32), 0.0),
    "all_nan": lambda: (np.full((4, 4, 4), np.nan, np.float32), 0.0),
    "inf": lambda: (np.where(np.random.default_rng(5).random((6, 7, 8)) < 0.1, np.float32(np.inf), R.noise_volume()[:6, :7, 30:38]).astype(np.float32), 0.0),
    "row130": lambda: (_row(130), 0.0),                                                   # a row that ends mid-chunk
    "row130_nan": lambda: (_row(130, nan=True), 0.0),
    "row62": lambda: (_row(62), 0.0), "row63": lambda: (_row(63), 0.0), "row64": lambda: (_row(64), 0.0), "row65": lambda: (_row(65), 0.0),
    "row125_nan": lambda: (_row(125, nan=True), 0.0),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    vol, level = VOLUMES[name]()
    verts, faces = R.marching_cubes(vol, level)
    for a in (vol, verts, faces):
        a.setflags(write=False)
    return vol, level, verts, faces


def _run(dev, name):
    from nr3d_lib_amd.bindings._marching_cubes import marching_cubes
    vol, level, verts, faces = reference(name)
    got_v, got_f = marching_cubes(torch.from_numpy(vol.copy()).to(dev), level)
    return got_v, got_f, torch.from_numpy(verts.copy()), torch.from_numpy(faces.copy())


@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_equals_restatement(dev, name):
    got_v, got_f, want_v, want_f = _run(dev, name)
    assert got_v.dtype == torch.float32 and got_f.dtype == torch.int64 and got_v.is_cuda and got_f.is_cuda
    assert tuple(got_v.shape) == tuple(want_v.shape) and tuple(got_f.shape) == tuple(want_f.shape), (got_v.shape, got_f.shape)
    if name in ("outside", "inside", "all_nan"):
        assert got_v.shape == (0, 3) and got_f.shape == (0, 3)
    assert torch.equal(got_f.cpu(), want_f)
    assert torch.equal(got_v.cpu(), want_v)


def test_poison_does_not_survive(dev):
    from nr3d_lib_amd import _hip as H
    assert H.POISON, "the GPU suite runs with NR3D_POISON_EMPTY=1 (tests/conftest.py)"
    for name in ("nan", "open", "row130_nan"):
        got_v, got_f, want_v, _ = _run(dev, name)
        assert not torch.isnan(got_v).any()
        assert int(got_f.min()) >= 0 and int(got_f.max()) < got_v.shape[0]
        assert not (got_f == -0x54545455).any()


def test_repeatable(dev):
    from nr3d_lib_amd.bindings._marching_cubes import marching_cubes
    vol = torch.from_numpy(R.nan_volume()).to(dev)
    a, b = marching_cubes(vol, 0.1), marching_cubes(vol, 0.1)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_errors(dev):
    from nr3d_lib_amd.bindings._marching_cubes import marching_cubes
    good = torch.zeros((4, 5, 6), device=dev)
    for bad in (good.cpu(), good.transpose(0, 2), good.double(), good[0], good[:1], good[:, :, :1]):
        with pytest.raises(RuntimeError):
            marching_cubes(bad)


# ---- graphics.trianglemesh on analytic SDFs ------------------------------------------------------------------------------------------------
RS, TR, Tr = 0.6, 0.55, 0.22


def sphere_sdf(x):
    return torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]) - RS


def torus_sdf(x):
    q = torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) - TR
    return torch.sqrt(q * q + x[:, 2] * x[:, 2]).unsqueeze(1) - Tr            # [n, 1]: both result shapes are accepted


def _sdf64(kind, p):
    p = p.astype(np.float64)
    if kind == "sphere":
        return np.linalg.norm(p, axis=1) - RS
    q = np.hypot(p[:, 0], p[:, 1]) - TR
    return np.hypot(q, p[:, 2]) - Tr


def _grad64(kind, p):
    p = p.astype(np.float64)
    if kind == "sphere":
        return p / np.linalg.norm(p, axis=1, keepdims=True)
    rho = np.hypot(p[:, 0], p[:, 1])
    q = rho - TR
    d = np.hypot(q, p[:, 2])
    return np.stack([q / d * p[:, 0] / rho, q / d * p[:, 1] / rho, p[:, 2] / d], 1)


@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_extract_mesh_tensors_analytic(dev, kind):
    from nr3d_lib_amd.graphics.trianglemesh import extract_mesh_tensors
    N = 33
    mesh = extract_mesh_tensors(sphere_sdf if kind == "sphere" else torus_sdf, level=0.0, N=N, chunk=5000, show_progress=False, device=dev)
    verts, faces, normals = (mesh[k].cpu().numpy() for k in ("verts", "faces", "normals"))
    assert mesh["colors"] is None
    assert mesh["stats"] == dict(nodes=N ** 3, nodes_queried=N ** 3, V=len(verts), F=len(faces), N=[N, N, N])
    assert len(verts) > 500 and R.is_closed_manifold(faces)
    assert R.euler(len(verts), faces) == (2 if kind == "sphere" else 0)
    assert R.signed_volume(verts, faces) > 0
    # a vertex is the zero of the linear interpolant of the SDF along a grid edge of length h: |sdf(v)| <= h^2 max|sdf''| / 8.  The second
    # derivatives of a distance function are the curvatures of its level sets: at the sphere 1 / 0.6; at the torus 1 / r = 1 / 0.22 around
    # the tube and at most 1 / (R - r) = 1 / 0.33 around the axis, so 1 / 0.22.
    h = 2.0 / (N - 1)
    bound = h * h / (8 * (RS if kind == "sphere" else Tr))
    err = np.abs(_sdf64(kind, verts)).max()
    print(f"{kind}: max |sdf(v)| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    dots = np.einsum("ij,ij->i", normals.astype(np.float64), _grad64(kind, verts))
    print(f"{kind}: min normal . gradient = {dots.min():.3f}")
    assert (dots > 0).all()
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-5)


def _occupancy(kind, res, aabb):
    lo, hi = np.array(aabb[0]), np.array(aabb[1])
    w = (hi - lo) / res
    c = [lo[a] + (np.arange(res) + 0.5) * w[a] for a in range(3)]
    p = np.stack(np.meshgrid(*c, indexing="ij"), -1).reshape(-1, 3)
    return (np.abs(_sdf64(kind, p)) <= 0.5 * np.linalg.norm(w)).reshape(res, res, res)


@pytest.mark.parametrize("kind,bmin,bmax,N", [("sphere", (-1., -1., -1.), (1., 1., 1.), 33), ("torus", (-1., -1., -1.), (1., 1., 1.), 33),
                                              ("sphere", (-1., -0.8, -0.7), (1., 0.9, 0.8), 24)])
def test_sparse_equals_dense(dev, kind, bmin, bmax, N):
    from nr3d_lib_amd.graphics.trianglemesh import extract_mesh_tensors
    fn = sphere_sdf if kind == "sphere" else torus_sdf
    aabb = [[-1., -1., -1.], [1., 1., 1.]]
    occ = torch.from_numpy(_occupancy(kind, 32, aabb)).to(dev)
    kw = dict(level=0.0, N=N, chunk=4096, show_progress=False, bmin=bmin, bmax=bmax, device=dev)
    dense = extract_mesh_tensors(fn, **kw)
    sparse = extract_mesh_tensors(fn, occ_grid=occ, occ_aabb=torch.tensor(aabb), **kw)
    assert dense["stats"]["V"] > 300
    assert torch.equal(sparse["verts"], dense["verts"]) and torch.equal(sparse["faces"], dense["faces"])
    assert sparse["stats"]["nodes_queried"] < sparse["stats"]["nodes"] == dense["stats"]["nodes_queried"]
    print(f"{kind} N={N}: {sparse['stats']['nodes_queried']} of {sparse['stats']['nodes']} nodes queried")
    # the resolution rule is the reference's formula
    size = np.array(bmax) - np.array(bmin)
    want_N = (size / size.min() * N).astype(np.int32)
    assert dense["stats"]["N"] == want_N.tolist() and dense["stats"]["nodes"] == int(want_N.prod())
    # and the vertices lie on the node lattice: index position * spacing + bmin
    spacing = size / (want_N - 1)
    idx = (dense["verts"].cpu().numpy().astype(np.float64) - np.array(bmin)) / spacing
    assert (np.abs(idx - np.round(idx)) < 1e-3).sum(1).min() >= 2


def test_extract_mesh_end_to_end(dev, tmp_path):
    from nr3d_lib_amd.graphics.trianglemesh import extract_mesh, extract_mesh_tensors, read_ply
    calls = []

    def color_fn(x, n):
        assert x.is_cuda and n.is_cuda and x.dim() == 2 and x.shape[1] == 3 and n.shape == x.shape
        assert torch.allclose(n.norm(dim=1), torch.ones(n.shape[0], device=n.device), atol=1e-5)
        calls.append(x.shape[0])
        return n * 0.5 + 0.5

    kw = dict(level=0.0, N=17, chunk=300, show_progress=False, device=dev)
    plain = extract_mesh_tensors(sphere_sdf, color_fn, include_color=True, **kw)
    V = plain["stats"]["V"]
    assert calls == [300] * (V // 300) + ([V % 300] if V % 300 else [])
    scale, offset = np.array([2.0, 1.0, 0.5], np.float32), np.array([0.25, -1.0, 3.0], np.float32)
    c, s = math.cos(0.3), math.sin(0.3)
    T = np.array([[c, -s, 0, 0.5], [s, c, 0, -2.0], [0, 0, 1, 1.0], [0, 0, 0, 1]], np.float32)
    path = str(tmp_path / "surface.ply")
    extract_mesh(sphere_sdf, color_fn, filepath=path, include_color=True, scale=scale, offset=offset, transform=T, **kw)
    back = read_ply(path)
    v = plain["verts"].cpu().numpy()
    want = (v * scale - offset) @ T[:3, :3].T + T[:3, 3]
    assert back["verts"].shape == (V, 3) and np.allclose(back["verts"], want, rtol=1e-5, atol=1e-5)
    assert np.array_equal(back["faces"], plain["faces"].cpu().numpy())
    # colours are queried before the transform, from the untransformed vertices and their normals
    assert np.array_equal(back["colors"], plain["colors"].cpu().numpy())
    assert np.array_equal(plain["colors"].cpu().numpy(), ((plain["normals"] * 0.5 + 0.5) * 255.).to(torch.uint8).cpu().numpy())
    # without colours: no colour properties
    extract_mesh(sphere_sdf, filepath=path, **kw)
    assert read_ply(path)["colors"] is None
