"""CPU: the marching-cubes case table (tools/gen_mc_table.py -> csrc/mc_table.inc), the numpy restatement of the output specification
(tests/marching_cubes_ref.py), the PLY writer / reader and the sparse node mask of nr3d_lib_amd/graphics/trianglemesh.py, and the header.

The table is common to the restatement and the kernels, so what catches a wrong table are the invariants asserted here on the restatement
(and on the device result in test_marching_cubes_gpu.py): closed, consistently oriented, Euler characteristic, positive volume."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import marching_cubes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the table --------------------------------------------------------------------------------------------------------------------
def test_table_is_what_the_generator_renders():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_table.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(os.path.join(ROOT, "nr3d_lib_amd", "csrc", "mc_table.inc")).read() == R.GEN.render()


def test_table_check_figures():
    assert R.TRI.shape == (256, 16) and R.TRI.dtype == np.int8 and R.NTRI.shape == (256,)
    assert R.NTRI.max() == 5 and R.NTRI.sum() == 820
    assert np.bincount(R.NTRI, minlength=6).tolist() == [2, 16, 50, 80, 76, 32]
    for case in range(256):
        row = R.TRI[case]
        n = 3 * R.NTRI[case]
        assert (row[:n] >= 0).all() and (row[:n] < 12).all() and (row[n:] == -1).all(), case


def test_table_uses_exactly_the_crossed_edges():
    for case in range(256):
        crossed = set()
        for e in range(12):
            p0, p1 = R.GEN.edge_ends(e)
            if ((case >> R.GEN.corner_id(p0)) & 1) != ((case >> R.GEN.corner_id(p1)) & 1):
                crossed.add(e)
        used = set(int(e) for e in R.TRI[case] if e >= 0)
        assert used == crossed, case
        # every triangle has three distinct edges
        for t in range(R.NTRI[case]):
            assert len(set(R.TRI[case, 3 * t:3 * t + 3].tolist())) == 3, case


def test_edge_numbering():
    """edge e = 4 a + u + 2 v, owned by its low end"""
    for e in range(12):
        p0, p1 = R.GEN.edge_ends(e)
        a = e >> 2
        assert p0[a] == 0 and p1[a] == 1 and R.GEN.edge_between(p0, p1) == e
        others = [d for d in range(3) if d != a]
        assert (p0[others[0]], p0[others[1]]) == (e & 1, (e >> 1) & 1)


# ---- 2. the restatement on analytic shapes ------------------------------------------------------------------------------------------------
def test_sphere():
    verts, faces = R.marching_cubes(R.sphere_volume())
    assert verts.shape == (576, 3) and faces.shape == (1148, 3) and verts.dtype == np.float32 and faces.dtype == np.int64
    assert R.is_closed_manifold(faces)
    assert R.euler(len(verts), faces) == 2
    # Volume, in index units (h = 1, r = 0.6 * 19 / 2 = 5.7).  Upper side: |p| - r is convex along an edge, so its linear interpolant lies
    # above it and vanishes where the function is <= 0: every vertex is inside the ball, so is the mesh (it lies in the convex hull of its
    # vertices): vol <= 4/3 pi r^3.  Lower side: a vertex misses the sphere by at most e = h^2 max f'' / 8 with f'' <= 1 / (r - h) on the
    # edge; a point q of a triangle with vertices at distance >= r - e and diameter D <= sqrt(3) h (one cell) has
    # |q|^2 >= (r - e)^2 - D^2 / 3 (variance identity, Jung), so the ball of that radius lies inside the closed mesh.
    r = 0.6 * 19 / 2
    e = 1.0 / (8 * (r - 1))
    r_in = math.sqrt((r - e) ** 2 - 1.0)
    vol = R.signed_volume(verts, faces)
    print(f"sphere volume {vol:.2f}, band [{4 / 3 * math.pi * r_in ** 3:.2f}, {4 / 3 * math.pi * r ** 3:.2f}]")
    assert vol > 0
    assert 4 / 3 * math.pi * r_in ** 3 <= vol <= 4 / 3 * math.pi * r ** 3
    # normals point outward: every vertex normal has a positive dot product with the radius
    n = R.vertex_normals(verts, faces)
    assert (np.einsum("ij,ij->i", n, verts.astype(np.float64) - 9.5) > 0).all()


def test_torus():
    verts, faces = R.marching_cubes(R.torus_volume())
    assert verts.shape == (600, 3) and faces.shape == (1200, 3)
    assert R.is_closed_manifold(faces)
    assert R.euler(len(verts), faces) == 0
    assert R.signed_volume(verts, faces) > 0


# ---- 3. noise: every case, closed and consistently oriented ------------------------------------------------------------------------------
def test_noise_all_cases_balanced():
    vol = R.noise_volume()
    assert vol.shape == (9, 11, 72)
    active, case = R.cell_state(vol, 0.0)
    assert active.all() and len(np.unique(case)) == 256
    verts, faces = R.marching_cubes(vol)
    assert verts.shape == (7268, 3) and faces.shape == (14972, 3)
    assert R.is_balanced(faces)
    # (not two faces per edge: on ambiguous faces a fan diagonal can coincide with a face segment)
    assert max(R.directed_edges(faces).values()) <= 2
    assert np.isfinite(verts).all()
    assert len(np.unique(faces)) == len(verts)
    # level 0.37 too
    v2, f2 = R.marching_cubes(vol, 0.37)
    assert R.is_balanced(f2) and len(np.unique(f2)) == len(v2)


@pytest.mark.parametrize("name", ["nan", "open"])
def test_open_meshes(name):
    """10 % NaN nodes / no padding: no vertex is unreferenced, every face index is valid, and a boundary edge borders an inactive or
    out-of-range cell"""
    vol = R.nan_volume() if name == "nan" else R.noise_volume(pad=False)
    verts, faces, edges, _ = R.marching_cubes(vol, details=True)
    assert len(verts) > 0 and len(faces) > 0
    assert faces.min() >= 0 and faces.max() < len(verts)
    assert len(np.unique(faces)) == len(verts)
    active, _ = R.cell_state(vol, 0.0)
    boundary = R.unbalanced_edges(faces)
    assert boundary, "an open mesh has boundary edges"

    def dead(c):
        return any(x < 0 or x >= n for x, n in zip(c, active.shape)) or not active[c]

    for a, b in boundary:
        common = R.edge_cells(edges[a, :3], edges[a, 3]) & R.edge_cells(edges[b, :3], edges[b, 3])
        assert common and any(dead(c) for c in common), (a, b)
    # and every face belongs to an active cell: all its vertices' edges touch one common active cell
    for f in faces[:: max(1, len(faces) // 500)]:
        common = set.intersection(*(R.edge_cells(edges[v, :3], edges[v, 3]) for v in f))
        assert any(not dead(c) for c in common)


def test_exact_level_values():
    """integer values in [-2, 2] with level 0: nodes exactly at the level are outside.  The owner is one end of the edge, so
    t = (level - v0) / (v1 - v0) is 0 when the owner sits at the level and 1 when the other end does (inside owner, v1 == level): t lies
    in [0, 1], and reaches 1 exactly in that case -- with these integers every other t is at most 2/3."""
    vol = R.exact_volume()
    assert (vol == 0).sum() > 50
    verts, faces, edges, t = R.marching_cubes(vol, details=True)
    assert np.isfinite(verts).all() and len(verts) > 0
    assert (t >= 0).all() and (t <= 1).all()
    hi = edges[:, :3].copy()
    hi[np.arange(len(edges)), edges[:, 3]] += 1
    v0, v1 = vol[tuple(edges[:, :3].T)], vol[tuple(hi.T)]
    assert ((t == 1) == (v1 == 0)).all() and ((t == 0) == (v0 == 0)).all()
    assert (t[(v1 != 0)] <= np.float32(2 / 3)).all()
    assert R.is_balanced(faces)
    assert len(np.unique(faces)) == len(verts)


# ---- 4. PLY ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_round_trip(tmp_path, with_colors):
    from nr3d_lib_amd.graphics.trianglemesh import export_ply, read_ply
    verts, faces = R.marching_cubes(R.sphere_volume())
    colors = np.random.default_rng(3).integers(0, 256, verts.shape, dtype=np.uint8) if with_colors else None
    path = str(tmp_path / "mesh.ply")
    export_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), None if colors is None else torch.from_numpy(colors))
    data = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 576\nproperty float x\nproperty float y\nproperty float z\n"
              + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if with_colors else "")
              + "element face 1148\nproperty list uchar int vertex_indices\nend_header\n")
    assert data.startswith(header.encode("ascii"))
    assert len(data) == len(header) + 576 * (15 if with_colors else 12) + 1148 * 13
    # the first vertex record and the first face record, byte for byte
    body = data[len(header):]
    assert body[:12] == verts[0].astype("<f4").tobytes()
    if with_colors:
        assert body[12:15] == colors[0].tobytes()
    fbody = body[576 * (15 if with_colors else 12):]
    assert fbody[:13] == b"\x03" + faces[0].astype("<i4").tobytes()
    back = read_ply(path)
    assert np.array_equal(back["verts"], verts) and np.array_equal(back["faces"], faces)
    assert (back["colors"] is None) if not with_colors else np.array_equal(back["colors"], colors)


def test_ply_empty_and_errors(tmp_path):
    from nr3d_lib_amd.graphics.trianglemesh import export_ply, read_ply
    path = str(tmp_path / "empty.ply")
    export_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    back = read_ply(path)
    assert back["verts"].shape == (0, 3) and back["faces"].shape == (0, 3)
    with pytest.raises(RuntimeError):
        export_ply(path, np.zeros((2, 3), np.float32), np.array([[0, 1, 2]]))


# ---- 5. header and ABI ---------------------------------------------------------------------------------------------------------------
def test_header_and_abi():
    from nr3d_lib_amd import _abi
    header = open(os.path.join(ROOT, "include", "nr3d_hip.h")).read()
    assert int(re.search(r"#define\s+NR3D_ABI_VERSION\s+(\d+)", header).group(1)) == 30 == _abi.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("nr3d_marching_cubes_count", 8), ("nr3d_marching_cubes_emit", 11), ("nr3d_marching_cubes_scratch_bytes", 3)):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == n_args, name
    assert _abi.SIGNATURES["nr3d_marching_cubes_scratch_bytes"][0] == "uint64_t"
    for name in ("nr3d_marching_cubes_count", "nr3d_marching_cubes_emit"):
        assert _abi.SIGNATURES[name][0] == "int" and _abi.SIGNATURES[name][1][-1] == "ptr"      # the stream comes last
    assert "marching_cubes.hip" in open(os.path.join(ROOT, "nr3d_lib_amd", "csrc", "Makefile")).read()


def test_binding_refuses_cpu_tensors():
    from nr3d_lib_amd.bindings._marching_cubes import marching_cubes
    with pytest.raises(RuntimeError):
        marching_cubes(torch.zeros(4, 4, 4))


# ---- 6. the sparse node mask ------------------------------------------------------------------------------------------------------------
def test_sparse_node_mask_covers_every_touching_cell():
    """brute force: 8^3 voxels over [-1, 1]^3, 13 x 17 x 11 nodes on a box that sticks out of it on one side: every corner of every cell that
    overlaps (closed boxes) an occupied voxel is selected"""
    from nr3d_lib_amd.graphics.trianglemesh import sparse_node_mask
    rng = np.random.default_rng(4)
    occ = np.zeros((8, 8, 8), bool)
    occ[tuple(rng.integers(0, 8, (3, 3)))] = True
    occ[0, 7, 3] = True                                     # one at the border
    bmin, bmax, N = np.array([-1.0, -1.2, -0.9]), np.array([1.0, 1.0, 1.1]), np.array([13, 17, 11])
    coords = [torch.linspace(float(bmin[a]), float(bmax[a]), int(N[a])) for a in range(3)]
    spacing = (bmax - bmin) / (N - 1)
    mask = sparse_node_mask(torch.from_numpy(occ), torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), coords, spacing, dilate=1).numpy()
    assert mask.shape == (13, 17, 11) and mask.dtype == bool
    assert 0 < mask.sum() < mask.size, "the mask must select something and not everything"
    c = [x.numpy().astype(np.float64) for x in coords]
    want = np.zeros(mask.shape, bool)
    for vx, vy, vz in np.argwhere(occ):
        lo = -1.0 + 0.25 * np.array([vx, vy, vz])
        hi = lo + 0.25
        hit = [np.nonzero((c[a][:-1] <= hi[a]) & (c[a][1:] >= lo[a]))[0] for a in range(3)]       # cells overlapping per axis
        for i in hit[0]:
            for j in hit[1]:
                for k in hit[2]:
                    want[i:i + 2, j:j + 2, k:k + 2] = True
    assert want.sum() > 0
    assert (mask | ~want).all(), f"{(want & ~mask).sum()} corners of touching cells are not selected"
    # dilate widens monotonically
    wider = sparse_node_mask(torch.from_numpy(occ), torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), coords, spacing, dilate=2).numpy()
    assert (wider | ~mask).all() and wider.sum() > mask.sum()
