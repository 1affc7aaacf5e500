"""nr3d_lib_amd.graphics.trianglemesh -- surface extraction from a trained SDF (nr3d_lib/graphics/trianglemesh.py:134-254 extract_mesh;
``load_obj`` / ``load_mat`` are not ported).

The reference builds the full [N^3, 3] coordinate tensor on the host, ships it to the device in chunks, copies every SDF value back into a
float64 numpy volume, runs ``skimage.measure.marching_cubes`` on one core and fills the PLY records in a Python loop over vertices.
Here the node coordinates are gathered on the device from three 1-D tables, the volume never leaves the device, the triangulation is
``bindings._marching_cubes`` (HIP, one readback), an occupancy grid can restrict the network queries to the nodes near the surface
(NaN marks the others), and the PLY file is written from numpy structured arrays.

    marching_cubes(volume, level, spacing, origin) -> verts, faces, normals             (device tensors)
    extract_mesh_tensors(query_sdf_fn, query_color_fn, ...) -> dict(verts, faces, normals, colors, stats)
    extract_mesh(query_sdf_fn, query_color_fn, *, filepath, ...)                          the reference's signature, + the sparse keywords
    export_ply / read_ply                                                                 binary_little_endian 1.0, the subset plyfile writes
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from ..bindings import _marching_cubes as _mc

__all__ = ["marching_cubes", "sparse_node_mask", "extract_mesh_tensors", "extract_mesh", "export_ply", "read_ply"]


def _vec3(v, device, name):
    t = torch.as_tensor(np.asarray(v, dtype=np.float32).reshape(-1), device=device)
    if t.numel() == 1:
        t = t.expand(3)
    if t.numel() != 3:
        raise RuntimeError(f"marching_cubes: `{name}` must have 3 components, got {t.numel()}")
    return t


def vertex_normals(verts, faces):
    """area-weighted vertex normals from the faces (``index_add_`` of the face cross products, then normalise); a vertex whose sum has
    zero length gets (0, 0, 1).  With the library's case table they point towards increasing value: outward for an SDF."""
    p0, p1, p2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    fn = torch.cross(p1 - p0, p2 - p0, dim=1)
    n = torch.zeros_like(verts)
    for k in range(3):
        n.index_add_(0, faces[:, k], fn)
    length = n.norm(dim=1, keepdim=True)
    unit = n / length.clamp_min(1e-30)
    fallback = torch.tensor([0.0, 0.0, 1.0], dtype=verts.dtype, device=verts.device)
    return torch.where(length > 0, unit, fallback)


def marching_cubes(volume, level=0., spacing=(1., 1., 1.), origin=(0., 0., 0.)):
    """volume float32 [Nx, Ny, Nz] on the GPU (NaN: node not evaluated) -> (verts float32 [V, 3] = index position * spacing + origin,
    faces int64 [F, 3], normals float32 [V, 3]), all on the device.

    Unlike ``skimage.measure.marching_cubes``, whose normals are finite differences of the volume, ``normals`` are the area-weighted
    vertex normals of the extracted faces; they point outward for an SDF.  Vertices and faces come in a canonical order (see
    include/nr3d_hip.h) and are the same bytes run after run."""
    verts, faces = _mc.marching_cubes(volume, level)
    verts = verts * _vec3(spacing, verts.device, "spacing") + _vec3(origin, verts.device, "origin")
    return verts, faces, vertex_normals(verts, faces)


def sparse_node_mask(occ_grid, occ_aabb, coords, spacing, dilate=1):
    """The nodes the sparse mode evaluates: bool [Nx, Ny, Nz].  occ_grid bool [Rx, Ry, Rz] over occ_aabb [2, 3]; coords: the three 1-D
    node coordinate tables; spacing [3].  A node is selected iff the occupancy voxel that contains it (index clamped into the grid) has
    an occupied voxel within D = dilate + ceil(max_a spacing_a / voxel_a) voxels (a max-pool of width 2 D + 1), so with dilate >= 1
    all 8 corners of any cell that touches an occupied voxel are selected.  Plain torch ops, on whatever device the grid is on."""
    dev = occ_grid.device
    if occ_grid.dim() != 3:
        raise RuntimeError(f"sparse_node_mask: `occ_grid` must be [Rx, Ry, Rz], got {list(occ_grid.shape)}")
    aabb = torch.as_tensor(occ_aabb, dtype=torch.float32).reshape(2, 3).cpu()
    res = torch.tensor(occ_grid.shape, dtype=torch.float32)
    voxel = (aabb[1] - aabb[0]) / res
    spacing = torch.as_tensor(np.asarray(spacing, dtype=np.float32)).reshape(3)
    D = int(dilate) + int(math.ceil(float((spacing / voxel).max())))
    near = F.max_pool3d(occ_grid[None, None].to(torch.float32), kernel_size=2 * D + 1, stride=1, padding=D)[0, 0] > 0
    idx = []
    for a in range(3):
        x = coords[a].to(device=dev, dtype=torch.float32)
        i = torch.floor((x - float(aabb[0, a])) / float(voxel[a])).to(torch.int64)
        idx.append(i.clamp_(0, occ_grid.shape[a] - 1))
    return near[idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]


def _progress(it, show, desc):
    if not show:
        return it
    try:
        from tqdm import tqdm
    except ImportError:
        return it
    return tqdm(it, desc=desc, leave=False)


def extract_mesh_tensors(query_sdf_fn, query_color_fn=None, *, level=0.0, N=512, chunk=16 * 1024, include_color=False,
                         show_progress=True, bmin=(-1., -1., -1.), bmax=(1., 1., 1.), device=torch.device('cuda'),
                         occ_grid=None, occ_aabb=None, dilate=1):
    """Marching cubes of ``query_sdf_fn`` on the box [bmin, bmax] -> dict(verts float32 [V, 3], faces int64 [F, 3], normals float32 [V, 3],
    colors uint8 [V, 3] or None, stats), tensors on ``device``.

    The grid is the reference's: an int N is the resolution of the shortest edge, ``(size / size.min() * N).astype(int32)``, spacing
    ``size / (N - 1)``, node coordinates ``torch.linspace(bmin, bmax, N)`` per axis.  ``query_sdf_fn(x [n, 3])`` returns [n] or [n, 1];
    ``query_color_fn(verts [n, 3], normals [n, 3])`` returns [n, 3] in [0, 1], stored as ``(out * 255).to(uint8)``.
    Sparse mode (``occ_grid`` bool [Rx, Ry, Rz] over ``occ_aabb`` [2, 3], e.g. an OccGridAccel's grid): only the nodes of
    ``sparse_node_mask`` are queried, the others stay NaN; cells away from the occupied voxels emit nothing.
    stats: dict(nodes, nodes_queried, V, F, N)."""
    device = torch.device(device)
    bmin_np, bmax_np = np.array(bmin, dtype=np.float64), np.array(bmax, dtype=np.float64)
    size = bmax_np - bmin_np
    if isinstance(N, (int, np.integer)) or len(N) == 1:
        n0 = int(N) if isinstance(N, (int, np.integer)) else int(N[0])
        N = (size / size.min() * n0).astype(np.int32)
    else:
        N = np.array(N)
    if N.shape != (3,) or (N < 2).any():
        raise RuntimeError(f"extract_mesh: the grid must have 3 dimensions of >= 2 nodes, got {N.tolist()}")
    spacing = size / (N - 1)
    nx, ny, nz = (int(n) for n in N)
    coords = [torch.linspace(float(bmin_np[a]), float(bmax_np[a]), int(N[a]), device=device) for a in range(3)]
    n_nodes = nx * ny * nz

    def node_xyz(idx):
        return torch.stack([coords[0][idx // (ny * nz)], coords[1][(idx // nz) % ny], coords[2][idx % nz]], dim=1)

    def query(idx):
        out = query_sdf_fn(node_xyz(idx))
        return out.reshape(-1).to(torch.float32)

    with torch.no_grad():
        if occ_grid is None:
            volume = torch.empty(n_nodes, dtype=torch.float32, device=device)
            for s in _progress(range(0, n_nodes, chunk), show_progress, "Querying surface"):
                e = min(s + chunk, n_nodes)
                volume[s:e] = query(torch.arange(s, e, device=device))
            n_queried = n_nodes
        else:
            if occ_aabb is None:
                raise RuntimeError("extract_mesh: `occ_grid` needs `occ_aabb` [2, 3]")
            mask = sparse_node_mask(occ_grid.to(device), occ_aabb, coords, spacing, dilate)
            sel = mask.reshape(-1).nonzero().squeeze(1)
            volume = torch.full((n_nodes,), float("nan"), dtype=torch.float32, device=device)
            for s in _progress(range(0, sel.numel(), chunk), show_progress, "Querying surface"):
                idx = sel[s:s + chunk]
                volume[idx] = query(idx)
            n_queried = int(sel.numel())
        verts, faces, normals = marching_cubes(volume.view(nx, ny, nz), level, spacing, bmin_np)
        colors = None
        if include_color:
            if query_color_fn is None:
                raise RuntimeError("extract_mesh: include_color=True needs `query_color_fn`")
            colors = torch.empty((verts.shape[0], 3), dtype=torch.uint8, device=device)
            for s in _progress(range(0, verts.shape[0], chunk), show_progress, "Querying color"):
                out = query_color_fn(verts[s:s + chunk], normals[s:s + chunk])
                colors[s:s + chunk] = (out * 255.).to(torch.uint8)
    stats = dict(nodes=n_nodes, nodes_queried=n_queried, V=int(verts.shape[0]), F=int(faces.shape[0]), N=[nx, ny, nz])
    return dict(verts=verts, faces=faces, normals=normals, colors=colors, stats=stats)


def extract_mesh(query_sdf_fn, query_color_fn=None, *, filepath='./surface.ply', level=0.0, N=512, chunk=16 * 1024,
                 include_color=False, show_progress=True, bmin=[-1., -1., -1.], bmax=[1., 1., 1.], offset=None, scale=None,
                 transform=None, device=torch.device('cuda'), occ_grid=None, occ_aabb=None, dilate=1):
    """The reference's ``extract_mesh``: marching cubes of ``query_sdf_fn`` on [bmin, bmax], optional vertex colours (queried BEFORE the
    vertex transform), then ``verts * scale``, ``verts - offset``, ``verts @ transform[:3, :3].T + transform[:3, 3]`` in this order, and a
    binary PLY file at ``filepath``.  ``occ_grid`` / ``occ_aabb`` / ``dilate``: the sparse mode of ``extract_mesh_tensors``.  Returns
    that function's dict with the transformed vertices (the reference returns None)."""
    mesh = extract_mesh_tensors(query_sdf_fn, query_color_fn, level=level, N=N, chunk=chunk, include_color=include_color,
                                show_progress=show_progress, bmin=bmin, bmax=bmax, device=device, occ_grid=occ_grid,
                                occ_aabb=occ_aabb, dilate=dilate)
    verts = mesh["verts"]
    if scale is not None:
        verts = verts * torch.as_tensor(np.array(scale, dtype=np.float32), device=verts.device)
    if offset is not None:
        verts = verts - torch.as_tensor(np.array(offset, dtype=np.float32), device=verts.device)
    if transform is not None:
        T = torch.as_tensor(np.array(transform, dtype=np.float32), device=verts.device)
        verts = verts @ T[:3, :3].T + T[:3, 3]
    mesh["verts"] = verts
    export_ply(filepath, verts, mesh["faces"], mesh["colors"])
    return mesh


# ---- PLY: binary_little_endian 1.0, what plyfile writes for the reference's record dtypes -------------------------------------------
_VERT_DTYPE = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
_COLOR_DTYPE = [("red", "u1"), ("green", "u1"), ("blue", "u1")]
_FACE_DTYPE = [("n", "u1"), ("vertex_indices", "<i4", (3,))]


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def ply_header(n_verts, n_faces, with_colors):
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n_verts}",
             "property float x", "property float y", "property float z"]
    if with_colors:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines += [f"element face {n_faces}", "property list uchar int vertex_indices", "end_header"]
    return "\n".join(lines) + "\n"


def export_ply(filepath, verts, faces, colors=None):
    """verts [V, 3] float, faces [F, 3] int (< 2^31), colors [V, 3] uint8 or None (tensors or arrays) -> a binary little-endian PLY with
    vertex properties ``float x y z`` (+ ``uchar red green blue``) and faces ``list uchar int vertex_indices``.  Vectorised: the records
    are numpy structured arrays."""
    verts, faces = _np(verts), _np(faces)
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise RuntimeError(f"export_ply: verts must be [V, 3] and faces [F, 3], got {list(verts.shape)} and {list(faces.shape)}")
    if faces.size and (faces.min() < 0 or faces.max() >= max(verts.shape[0], 1) or faces.max() >= 2 ** 31):
        raise RuntimeError("export_ply: a face index outside [0, V)")
    vrec = np.empty(verts.shape[0], dtype=_VERT_DTYPE + (_COLOR_DTYPE if colors is not None else []))
    for k, name in enumerate("xyz"):
        vrec[name] = verts[:, k]
    if colors is not None:
        colors = _np(colors)
        if colors.shape != verts.shape or colors.dtype != np.uint8:
            raise RuntimeError(f"export_ply: colors must be uint8 {list(verts.shape)}, got {colors.dtype} {list(colors.shape)}")
        for k, (name, _) in enumerate(_COLOR_DTYPE):
            vrec[name] = colors[:, k]
    frec = np.empty(faces.shape[0], dtype=_FACE_DTYPE)
    frec["n"] = 3
    frec["vertex_indices"] = faces
    with open(filepath, "wb") as f:
        f.write(ply_header(verts.shape[0], faces.shape[0], colors is not None).encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def read_ply(filepath):
    """the reader of exactly the subset ``export_ply`` writes -> dict(verts float32 [V, 3], faces int64 [F, 3], colors uint8 [V, 3] or
    None) as numpy arrays"""
    data = open(filepath, "rb").read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise RuntimeError(f"read_ply: {filepath} is not a PLY file")
    header = data[:end + len(b"end_header\n")].decode("ascii")
    lines = header.split("\n")
    if lines[1] != "format binary_little_endian 1.0":
        raise RuntimeError(f"read_ply: {lines[1]!r}, only binary_little_endian 1.0 is read")
    n_verts, n_faces = int(lines[2].split()[2]), None
    with_colors = "property uchar red" in lines
    for ln in lines:
        if ln.startswith("element face "):
            n_faces = int(ln.split()[2])
    if header != ply_header(n_verts, n_faces, with_colors):
        raise RuntimeError(f"read_ply: {filepath} has a header outside the subset export_ply writes")
    vdt = np.dtype(_VERT_DTYPE + (_COLOR_DTYPE if with_colors else []))
    fdt = np.dtype(_FACE_DTYPE)
    body = data[len(header):]
    if len(body) != n_verts * vdt.itemsize + n_faces * fdt.itemsize:
        raise RuntimeError(f"read_ply: {filepath} has {len(body)} body bytes, the header announces {n_verts * vdt.itemsize + n_faces * fdt.itemsize}")
    vrec = np.frombuffer(body, dtype=vdt, count=n_verts)
    frec = np.frombuffer(body, dtype=fdt, count=n_faces, offset=n_verts * vdt.itemsize)
    if n_faces and (frec["n"] != 3).any():
        raise RuntimeError(f"read_ply: {filepath} has a face that is not a triangle")
    verts = np.stack([vrec["x"], vrec["y"], vrec["z"]], 1).astype(np.float32)
    colors = np.stack([vrec["red"], vrec["green"], vrec["blue"]], 1) if with_colors else None
    return dict(verts=verts, faces=frec["vertex_indices"].astype(np.int64), colors=colors)
