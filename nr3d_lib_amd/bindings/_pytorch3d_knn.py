"""nr3d_lib_amd.bindings._pytorch3d_knn -- the twin of the reference's pybind module ``nr3d_lib.bindings._pytorch3d_knn`` (externals/
pytorch3d_knn) over csrc/knn.hip through include/nr3d_hip.h: brute-force k nearest neighbours between two batched point clouds, and the
backward.  ``nr3d_lib_amd.maths.pytorch3d_knn`` is its caller.

The kernel's result is already what the reference's Python wrapper makes of its kernel's: sorted by (distance, index), zero-padded where a
p2 cloud is shorter than K and in the rows past ``lengths1``.  ``version`` is accepted and ignored (one implementation per (D, K)).
float32 ONLY: the reference's float64 forward is not rebuilt, any other dtype raises a RuntimeError that names float32.  ``lengths1`` /
``lengths2`` stay on the device (the kernels read them): no host sync anywhere.  A CPU tensor raises; the pure-torch route for CPU
tensors lives in ``maths.pytorch3d_knn``."""
import torch

from .. import _hip as H
from ._args import chk, same_device

__all__ = ["knn_points_idx", "knn_points_backward", "TILE", "fast_path", "launch_plan"]


def TILE(D):
    """p2 points per LDS tile of the fast kernel for dimension D (0: no fast kernel for this D)"""
    return int(H.lib().nr3d_knn_tile_points(int(D)))


def fast_path(D, K):
    """True: k_knn<D, KB, NORM> serves (D, K); False: the generic, unoptimised k_knn_any"""
    return bool(H.lib().nr3d_knn_fast_path(int(D), int(K)))


def launch_plan(N, P1, D, K):
    """(R, wg) of the k_knn<D, KB, NORM, R> launch for N clouds of P1 query points: R queries per lane, wg lanes per workgroup, from the
    function the launcher itself calls; None: the generic k_knn_any serves (D, K)"""
    plan = int(H.lib().nr3d_knn_launch_plan(int(N), int(P1), int(D), int(K)))
    return (plan & 0xFF, plan >> 8) if plan else None


def _clouds(fn, p1, p2, lengths1, lengths2, norm):
    for name, t in (("p1", p1), ("p2", p2)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{fn}: `{name}` must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{fn}: `{name}` must be float32 (the only dtype of the HIP kernels), got {t.dtype}")
        chk(fn, name, t)
        if t.dim() != 3:
            raise RuntimeError(f"{fn}: `{name}` must be [N, P, D], got {list(t.shape)}")
    N, P1, D = p1.shape
    if p2.shape[0] != N or p2.shape[2] != D:
        raise RuntimeError(f"{fn}: `p2` must be [{N}, P2, {D}] like `p1` {list(p1.shape)}, got {list(p2.shape)}")
    P2 = p2.shape[1]
    if norm not in (1, 2):
        raise RuntimeError(f"{fn}: norm = {norm!r}, 1 (L1) or 2 (squared L2)")
    if D < 1:
        raise RuntimeError(f"{fn}: D = 0, at least one coordinate")
    if P1 >= 2 ** 31 or P2 >= 2 ** 31:
        raise RuntimeError(f"{fn}: P1 = {P1}, P2 = {P2} points per cloud, the limit is 2^31 - 1 each")
    for name, t in (("lengths1", lengths1), ("lengths2", lengths2)):
        if t is not None:
            chk(fn, name, t, shape=(N,), dtype=torch.int64)
    same_device(fn, p1.device, "p1", p2=p2, lengths1=lengths1, lengths2=lengths2)
    return N, P1, P2, D


def knn_points_idx(p1, p2, lengths1, lengths2, norm, K, version=-1):
    """p1 float32 [N, P1, D], p2 float32 [N, P2, D], lengths int64 [N] or None -> (idx int64 [N, P1, K], dists float32 [N, P1, K]) by the
    contract of include/nr3d_hip.h (sorted, padded with zeros)"""
    fn = "knn_points_idx"
    N, P1, P2, D = _clouds(fn, p1, p2, lengths1, lengths2, norm)
    K = int(K)
    if K < 1:
        raise RuntimeError(f"{fn}: K = {K}, at least one neighbour")
    dev = p1.device
    if N == 0 or P1 == 0 or P2 == 0:
        return torch.zeros((N, P1, K), dtype=torch.int64, device=dev), torch.zeros((N, P1, K), dtype=torch.float32, device=dev)
    with H.on_device(dev):
        dists = H.empty((N, P1, K), dtype=torch.float32, device=dev)
        idx = H.empty((N, P1, K), dtype=torch.int64, device=dev)
        H.check(H.lib().nr3d_knn_points(H.ptr(p1), H.ptr(p2), H.ptr(lengths1), H.ptr(lengths2), N, P1, P2, D, K, int(norm), H.ptr(dists),
                                        H.ptr(idx), H.stream_of(p1)))
    return idx, dists


def knn_points_backward(p1, p2, lengths1, lengths2, idx, norm, grad_dists):
    """-> (grad_p1 float32 [N, P1, D], grad_p2 float32 [N, P2, D]); idx and grad_dists [N, P1, K] as the forward shaped them"""
    fn = "knn_points_backward"
    N, P1, P2, D = _clouds(fn, p1, p2, lengths1, lengths2, norm)
    chk(fn, "idx", idx, dtype=torch.int64)
    if idx.dim() != 3 or tuple(idx.shape[:2]) != (N, P1) or idx.shape[2] < 1:
        raise RuntimeError(f"{fn}: `idx` must be [{N}, {P1}, K] with K >= 1, got {list(idx.shape)}")
    K = idx.shape[2]
    if isinstance(grad_dists, torch.Tensor) and grad_dists.dtype != torch.float32:
        raise RuntimeError(f"{fn}: `grad_dists` must be float32 (the only dtype of the HIP kernels), got {grad_dists.dtype}")
    chk(fn, "grad_dists", grad_dists, shape=(N, P1, K))
    dev = p1.device
    same_device(fn, dev, "p1", idx=idx, grad_dists=grad_dists)
    grad_p2 = torch.zeros((N, P2, D), dtype=torch.float32, device=dev)
    if N == 0 or P1 == 0 or P2 == 0:
        return torch.zeros((N, P1, D), dtype=torch.float32, device=dev), grad_p2
    with H.on_device(dev):
        grad_p1 = H.empty((N, P1, D), dtype=torch.float32, device=dev)
        H.check(H.lib().nr3d_knn_points_backward(H.ptr(p1), H.ptr(p2), H.ptr(lengths1), H.ptr(lengths2), H.ptr(idx), H.ptr(grad_dists), N, P1,
                                                 P2, D, K, int(norm), H.ptr(grad_p1), H.ptr(grad_p2), H.stream_of(p1)))
    return grad_p1, grad_p2
