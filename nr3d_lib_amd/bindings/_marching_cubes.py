"""nr3d_lib_amd.bindings._marching_cubes -- marching cubes on a device volume (csrc/marching_cubes.hip through include/nr3d_hip.h): one
vertex per live edge, the triangles of the generated case table, both in the canonical order of the header, bit for bit what
tests/marching_cubes_ref.py restates.

Like ``_nerfpp_march`` this module has NO reference twin: the reference copies the volume to the host and calls
``skimage.measure.marching_cubes`` (nr3d_lib/graphics/trianglemesh.py:210-214).  ``graphics.trianglemesh`` is its caller.  Count (per
z-row: live edges, triangles; two scans; V and F into pinned words: the ONE device->host sync) -> emit (vertices and per-node vertex
words, then the faces).  A CPU tensor raises RuntimeError; there is no fallback here, and no backward."""
import torch

from .. import _hip as H
from ._args import chk

__all__ = ["marching_cubes"]


def marching_cubes(volume, level=0.0):
    """volume float32 [Nx, Ny, Nz] contiguous on the GPU, every dimension >= 2; NaN marks nodes that were not evaluated (a cell with a
    non-finite corner emits nothing).  -> (verts float32 [V, 3] in INDEX units, faces int64 [F, 3]); two empty tensors when V == 0."""
    fn = "marching_cubes"
    chk(fn, "volume", volume)
    if volume.dim() != 3 or min(volume.shape) < 2:
        raise RuntimeError(f"{fn}: `volume` must be [Nx, Ny, Nz] with every dimension >= 2, got {list(volume.shape)}")
    Nx, Ny, Nz = volume.shape
    if Nx * Ny >= 2 ** 28 or Nx * Ny * Nz >= 2 ** 36:
        raise RuntimeError(f"{fn}: {Nx} x {Ny} x {Nz} nodes, the limits are 2^28 - 1 z-rows and 2^36 - 1 nodes per call (split the volume)")
    dev, level = volume.device, float(level)
    with H.on_device(dev):
        l, st = H.lib(), H.stream_of(volume)
        nbytes = int(l.nr3d_marching_cubes_scratch_bytes(Nx, Ny, Nz))
        scratch = H.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        totals = H.host_i64(2, dev)
        H.check(l.nr3d_marching_cubes_count(H.ptr(volume), Nx, Ny, Nz, level, H.ptr(scratch), H.ptr(totals), st))
        V, F = H.wait_i64(totals, dev)                      # the one device->host sync
        if V >= 2 ** 29:
            raise RuntimeError(f"{fn}: {V} vertices, the limit is 2^29 - 1 per call (split the volume)")
        verts = H.empty((V, 3), dtype=torch.float32, device=dev)
        faces = H.empty((F, 3), dtype=torch.int64, device=dev)
        if V:
            H.check(l.nr3d_marching_cubes_emit(H.ptr(volume), Nx, Ny, Nz, level, H.ptr(scratch), V, F, H.ptr(verts), H.ptr(faces), st))
    return verts, faces
