"""tests/marching_cubes_ref.py -- the numpy restatement of the marching-cubes specification of include/nr3d_hip.h, and the mesh
invariants the tests assert.  It reads the case table from tools/gen_mc_table.py, so table errors are common to it and the kernels: the
invariants (closed, consistently oriented, Euler characteristic, outward normals, positive volume) are what catch those.

    node inside iff v < level, outside iff v >= level (NaN neither); cell active iff its 8 corners are finite
    edge live iff one end inside, the other outside, and one of its up to four incident cells is active: one vertex per live edge
    vertex order: owner node linear (x slowest, z fastest), then axis; position = owner index + (level - v0) / (v1 - v0) on the axis
    face order: cells linear, then table order
All float32 arithmetic is numpy float32: one subtraction, one subtraction, one division, one addition."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_mc_table
    finally:
        sys.path.pop(0)
    return gen_mc_table


GEN = _generator()
TRI, NTRI = GEN.tables()
EDGE_P0 = np.array([GEN.edge_ends(e)[0] for e in range(12)], np.int64)       # offset of the owner node
EDGE_AXIS = np.arange(12) >> 2


def _cells(a):
    """[Nx-1, Ny-1, Nz-1, 8]: the 8 corners of every cell, corner c at offsets (c & 1, (c >> 1) & 1, (c >> 2) & 1)"""
    nx, ny, nz = a.shape
    return np.stack([a[(c & 1):nx - 1 + (c & 1), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), ((c >> 2) & 1):nz - 1 + ((c >> 2) & 1)]
                     for c in range(8)], -1)


def cell_state(vol, level):
    """(active bool [cells], case int [cells])"""
    level = np.float32(level)
    active = _cells(np.isfinite(vol)).all(-1)
    case = (_cells(vol < level).astype(np.int64) << np.arange(8)).sum(-1)
    return active, case


def marching_cubes(vol, level=0.0, details=False):
    """vol float32 [Nx, Ny, Nz] -> (verts float32 [V, 3] in index units, faces int64 [F, 3]); details: also (edges int [V, 4]: owner
    node and axis of every vertex, t float32 [V]: its parameter on the edge)"""
    vol = np.ascontiguousarray(vol, np.float32)
    assert vol.ndim == 3 and min(vol.shape) >= 2
    level = np.float32(level)
    shape = np.array(vol.shape)
    with np.errstate(invalid="ignore"):
        inside, outside = vol < level, vol >= level
        active, case = cell_state(vol, level)
    live = np.zeros(vol.shape + (3,), bool)
    tpar = np.zeros(vol.shape + (3,), np.float32)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = (inside[lo] & outside[hi]) | (outside[lo] & inside[hi])
        # the edge of owner p along a touches the cells p - (offsets in the two other dimensions)
        pad = [(1, 1)] * 3
        pad[a] = (0, 0)
        ap = np.pad(active, pad)
        o1, o2 = [d for d in range(3) if d != a]
        anycell = np.zeros(cross.shape, bool)
        for s1 in (0, 1):
            for s2 in (0, 1):
                sl = [slice(None)] * 3
                sl[o1] = slice(s1, s1 + shape[o1])
                sl[o2] = slice(s2, s2 + shape[o2])
                anycell |= ap[tuple(sl)]
        live[lo + (a,)] = cross & anycell
        with np.errstate(all="ignore"):
            v0, v1 = vol[lo], vol[hi]
            tpar[lo + (a,)] = (level - v0) / (v1 - v0)
    flat = live.reshape(-1)
    vid = (np.cumsum(flat) - flat).reshape(live.shape)                          # the id a live edge gets
    where = np.argwhere(live)                                                   # (i, j, k, axis) in vertex order
    verts = where[:, :3].astype(np.float32)
    verts[np.arange(len(where)), where[:, 3]] += tpar[live]
    # faces
    ntri = np.where(active, NTRI[case], 0)
    cells = np.argwhere(ntri > 0)
    cs = case[ntri > 0]
    edges = TRI[cs][:, :15].reshape(-1, 5, 3).astype(np.int64)                   # [n, 5, 3] edge ids, -1 padded
    keep = edges[:, :, 0] >= 0
    owner = cells[:, None, None, :] + EDGE_P0[np.maximum(edges, 0)]              # [n, 5, 3, 3]
    ids = vid[owner[..., 0], owner[..., 1], owner[..., 2], EDGE_AXIS[np.maximum(edges, 0)]]
    assert live[owner[..., 0], owner[..., 1], owner[..., 2], EDGE_AXIS[np.maximum(edges, 0)]][keep].all()
    faces = ids[keep].astype(np.int64).reshape(-1, 3)
    if details:
        return verts, faces, where, tpar[live]
    return verts, faces


def edge_cells(owner, axis):
    """the (up to four, possibly out-of-range) cells around the edge of `owner` along `axis`, as a set of index triples"""
    o1, o2 = [d for d in range(3) if d != axis]
    out = set()
    for s1 in (0, 1):
        for s2 in (0, 1):
            c = list(int(x) for x in owner)
            c[o1] -= s1
            c[o2] -= s2
            out.add(tuple(c))
    return out


def unbalanced_edges(faces):
    d = directed_edges(faces)
    return [(a, b) for (a, b), n in d.items() if d.get((b, a), 0) != n]


# ---- invariants ----------------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    """{(a, b): count} over the three directed edges of every face"""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    u, c = np.unique(e, axis=0, return_counts=True)
    return {(int(a), int(b)): int(n) for (a, b), n in zip(u, c)}


def is_balanced(faces):
    """every directed edge occurs as often as its reverse: closed and consistently oriented"""
    d = directed_edges(faces)
    return all(d.get((b, a), 0) == n for (a, b), n in d.items())


def is_closed_manifold(faces):
    """every undirected edge lies in exactly 2 faces; every directed edge occurs once and so does its reverse"""
    d = directed_edges(faces)
    return all(n == 1 and d.get((b, a), 0) == 1 for (a, b), n in d.items())


def euler(n_verts, faces):
    d = directed_edges(faces)
    n_edges = len({(min(a, b), max(a, b)) for a, b in d})
    return n_verts - n_edges + len(faces)


def signed_volume(verts, faces):
    p = verts.astype(np.float64)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def vertex_normals(verts, faces):
    p = verts.astype(np.float64)
    n = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    out = np.zeros_like(p)
    for k in range(3):
        np.add.at(out, faces[:, k], n)
    return out


# ---- volumes the CPU and the GPU tests share ------------------------------------------------------------------------------------------
def grid(n, lo=-1.0, hi=1.0):
    g = np.linspace(lo, hi, n, dtype=np.float32)
    return np.meshgrid(g, g, g, indexing="ij")


def sphere_volume(n=20, r=0.6):
    x, y, z = grid(n)
    return (np.sqrt(x * x + y * y + z * z) - np.float32(r)).astype(np.float32)


def torus_volume(n=20, R=0.55, r=0.22):
    x, y, z = grid(n)
    q = np.sqrt(x * x + y * y) - np.float32(R)
    return (np.sqrt(q * q + z * z) - np.float32(r)).astype(np.float32)


def noise_volume(pad=True):
    v = np.random.default_rng(0).standard_normal((7, 9, 70)).astype(np.float32)
    return np.pad(v, 1, constant_values=1.0) if pad else v


def nan_volume():
    v = noise_volume()
    v[np.random.default_rng(1).random(v.shape) < 0.1] = np.nan
    return v


def exact_volume():
    v = np.random.default_rng(2).integers(-2, 3, (8, 8, 8)).astype(np.float32)
    return np.pad(v, 1, constant_values=1.0)
