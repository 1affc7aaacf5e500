"""nr3d_lib_amd.maths.pytorch3d_knn -- ``knn_points`` and ``knn_gather`` with the names, signatures and results of the reference's
``nr3d_lib.maths.pytorch3d_knn`` (borrowed there from pytorch3d: Ravi et al., "Accelerating 3D Deep Learning with PyTorch3D",
arXiv:2007.08501), on the HIP kernel of csrc/knn.hip.

What differs from the reference, none of it in the results:
  * The kernel's output is already sorted by (distance, index) and zero-padded (include/nr3d_hip.h), so the wrapper's ``lengths2.min() <
    K`` read-back and its sort / gather are not reproduced; ``return_sorted=False`` returns the same, sorted, result.  Among equal
    distances the lower index comes first, and the order is the same run after run.
  * ``version`` is accepted and ignored: there is one implementation per (D, K).
  * ``knn_gather`` applies the pad mask with ``torch.where`` unconditionally (the reference's ``lengths.min() < K`` branch is a host
    sync); ``M == 0`` returns zeros.
  * float32 only: the reference's float64 forward is not rebuilt; any other dtype is a RuntimeError that names float32.
  * Non-finite coordinates, or finite ones so large that a float32 distance overflows to inf: the neighbours of such a row are
    unspecified (indices stay in range).
  * No double backward (the reference is ``once_differentiable`` too).

CPU tensors take a pure-torch route with the same contract (``_knn_torch``: explicit differences, chunked over P1 so that a chunk's
[rows, P2] matrix stays under ``CHUNK_BYTES``, neighbours from a stable sort, the backward by index).  On the float32 lattice of
tests/knn_ref.py it gives the kernel's bits; elsewhere its squares are rounded before they are added where the kernel fuses them
(the last bit of a distance may differ).  The same route runs on GPU tensors while ``FUSED_KNN`` is False: the A/B partner of
tools/exp_knn.py and a second implementation for the tests.  profiles/knn.json has the fast kernel (D <= 8, K <= 32) ahead of it in
every measured row, by 22x to 409x (2^20 x 2^20, where the torch route was too slow to run, is estimated), so ``FUSED_KNN`` is True; the generic kernel that serves every other (D, K) is unoptimised and
loses to the torch route while the query rows are too few to fill the GPU, so with ``FUSED_KNN`` True such a call takes the kernel
only from ``GENERIC_MIN_ROWS`` query rows (N P1) on, a gate by size like the marcher's lanes-per-ray choice; 0 sends everything to
the kernel (the tests do that)."""
from collections import namedtuple
from typing import Union

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

__all__ = [
    'knn_points',
    'knn_gather'
]

_KNN = namedtuple("KNN", "dists idx knn")

FUSED_KNN = True            # GPU tensors: True = the HIP kernel, False = the pure-torch route (module attribute: measurement and tests)
# (D, K) off the fast kernel: the generic kernel from this many query rows (N P1) on, the torch route below.  A single-point fit: measured at
# D = 3, K = 40, P2 = 2^14 only (profiles/knn.json: torch ahead at 2^15 rows, the kernel from 2^16); the crossover moves with P2 (the torch
# route's sort) and K (the kernel's insertion), which the gate does not look at.  The two routes differ in arithmetic off the lattice: the
# kernel's norm 2 is the fmaf chain of the contract, the torch route rounds every square before it adds it, so for such a (D, K) the last bit
# of a distance, and with it the order of a near tie, can depend on which side of the gate N P1 falls (2 to 14 of 10^5 to 10^7 indices in
# profiles/knn.json).  Set it to 0 for the kernel's arithmetic at every size.
GENERIC_MIN_ROWS = 1 << 16
CHUNK_BYTES = 1 << 26       # the pure-torch route: bytes of one chunk's float32 [rows, P2] distance matrix


def _check(fn, p1, p2, lengths1, lengths2, norm):
    for name, t in (("p1", p1), ("p2", p2)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{fn}: `{name}` must be float32 (the reference's float64 forward is not rebuilt), got {t.dtype}")
    for name, t in (("lengths1", lengths1), ("lengths2", lengths2)):
        if t.dtype != torch.int64 or tuple(t.shape) != (p1.shape[0],):
            raise RuntimeError(f"{fn}: `{name}` must be int64 [{p1.shape[0]}], got {t.dtype} {list(t.shape)}")
        if t.device != p1.device:
            raise RuntimeError(f"{fn}: `{name}` is on {t.device}, p1 on {p1.device}")
    if p2.device != p1.device:
        raise RuntimeError(f"{fn}: `p2` is on {p2.device}, p1 on {p1.device}")


def _knn_torch(p1, p2, lengths1, lengths2, norm, K):
    """the contract of include/nr3d_hip.h in torch ops -> (idx, dists); no host sync"""
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    dev = p1.device
    dists = torch.zeros((N, P1, K), dtype=torch.float32, device=dev)
    idx = torch.zeros((N, P1, K), dtype=torch.int64, device=dev)
    if N == 0 or P1 == 0 or P2 == 0:
        return idx, dists
    len1, len2 = lengths1.clamp(0, P1), lengths2.clamp(0, P2)
    k = min(K, P2)
    rows = max(1, CHUNK_BYTES // (4 * P2 * N))
    dead2 = torch.arange(P2, device=dev)[None, None, :] >= len2[:, None, None]                 # [N, 1, P2]
    pad = (torch.arange(k, device=dev)[None, None, :] >= len2[:, None, None])                 # [N, 1, k]
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    for i0 in range(0, P1, rows):
        a = p1[:, i0:i0 + rows]
        d = a[:, :, None, 0] - p2[:, None, :, 0]
        dist = d * d if norm == 2 else d.abs()
        for c in range(1, D):
            d = a[:, :, None, c] - p2[:, None, :, c]
            dist = dist + (d * d if norm == 2 else d.abs())
        dist = torch.where(dead2, inf, dist)
        sd, si = torch.sort(dist, dim=2, stable=True)
        dead = pad | (torch.arange(i0, i0 + a.shape[1], device=dev)[None, :, None] >= len1[:, None, None])
        dists[:, i0:i0 + rows, :k] = torch.where(dead, torch.zeros((), dtype=torch.float32, device=dev), sd[:, :, :k])
        idx[:, i0:i0 + rows, :k] = torch.where(dead, torch.zeros((), dtype=torch.int64, device=dev), si[:, :, :k])
    return idx, dists


def _knn_torch_backward(p1, p2, lengths1, lengths2, idx, norm, grad_dists):
    """the backward of include/nr3d_hip.h by index -> (grad_p1, grad_p2)"""
    N, P1, D = p1.shape
    P2, K = p2.shape[1], idx.shape[2]
    dev = p1.device
    grad_p2 = torch.zeros((N, P2, D), dtype=torch.float32, device=dev)
    if N == 0 or P1 == 0 or P2 == 0:
        return torch.zeros((N, P1, D), dtype=torch.float32, device=dev), grad_p2
    live = (torch.arange(K, device=dev)[None, None, :] < lengths2.clamp(0, P2)[:, None, None]) \
        & (torch.arange(P1, device=dev)[None, :, None] < lengths1.clamp(0, P1)[:, None, None])           # [N, P1, K]
    live = live & (idx >= 0) & (idx < P2)              # an idx outside [0, P2) is skipped: its t is zero, the clamp only keeps the gather in range
    j = idx.clamp(0, P2 - 1)
    nb = torch.gather(p2[:, :, None, :].expand(-1, -1, K, -1), 1, j[..., None].expand(-1, -1, -1, D))   # [N, P1, K, D]
    g = grad_dists[..., None]
    a = p1[:, :, None, :]
    t = (2.0 * g) * (a - nb) if norm == 2 else torch.where(a > nb, g, -g)
    t = torch.where(live[..., None], t, torch.zeros((), dtype=torch.float32, device=dev))
    grad_p1 = t[:, :, 0]
    for k in range(1, K):
        grad_p1 = grad_p1 + t[:, :, k]
    grad_p2.view(N * P2, D).index_add_(0, (j + P2 * torch.arange(N, device=dev)[:, None, None]).reshape(-1), (-t).reshape(-1, D))
    return grad_p1.contiguous(), grad_p2


def _fused(p1, K=None):
    """the kernel route?  K None: the backward, which has one kernel for every (D, K)"""
    if not (p1.is_cuda and FUSED_KNN):
        return False
    if K is None or p1.shape[0] * p1.shape[1] >= GENERIC_MIN_ROWS:
        return True
    from ..bindings import _pytorch3d_knn as _C
    return _C.fast_path(p1.shape[2], K)


class _knn_points(Function):
    """(dists, idx) of the k-NN contract with its once-differentiable backward: the HIP binding for GPU tensors, the pure-torch route for
    CPU tensors (and for GPU tensors that ``_fused`` sends there).  ``idx`` carries no gradient."""

    @staticmethod
    def forward(ctx, p1, p2, lengths1, lengths2, K, norm):
        _check("knn_points", p1, p2, lengths1, lengths2, norm)
        K = int(K)
        if K < 1:
            raise RuntimeError(f"knn_points: K = {K}, at least one neighbour")
        if _fused(p1, K):
            from ..bindings import _pytorch3d_knn as _C
            idx, dists = _C.knn_points_idx(p1, p2, lengths1, lengths2, norm, K, -1)
        else:
            idx, dists = _knn_torch(p1, p2, lengths1, lengths2, norm, K)
        ctx.norm = norm
        ctx.save_for_backward(p1, p2, lengths1, lengths2, idx)
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dists, _grad_idx):
        p1, p2, lengths1, lengths2, idx = ctx.saved_tensors
        g = grad_dists.to(torch.float32).contiguous()
        if _fused(p1):
            from ..bindings import _pytorch3d_knn as _C
            grads = _C.knn_points_backward(p1, p2, lengths1, lengths2, idx, ctx.norm, g)
        else:
            grads = _knn_torch_backward(p1, p2, lengths1, lengths2, idx, ctx.norm, g)
        return (*grads, None, None, None, None)


def knn_points(
    p1: torch.Tensor,
    p2: torch.Tensor,
    lengths1: Union[torch.Tensor, None] = None,
    lengths2: Union[torch.Tensor, None] = None,
    norm: int = 2,
    K: int = 1,
    version: int = -1,
    return_nn: bool = False,
    return_sorted: bool = True,
) -> _KNN:
    """For every point of ``p1`` the ``K`` nearest points of ``p2`` within the same batch element.

    p1 float32 [N, P1, D] and p2 float32 [N, P2, D]; ``lengths1`` / ``lengths2`` int64 [N] say how many leading points of each cloud
    count (None: all of them).  ``norm`` 2 measures squared Euclidean distance, 1 the sum of absolute differences.  ``version`` and
    ``return_sorted`` belong to the reference's signature and change nothing here: there is one implementation per (D, K) and its
    result is always sorted.

    Returns ``KNN(dists, idx, knn)``: ``dists`` float32 [N, P1, K] ascending, ``idx`` int64 [N, P1, K] with ``p2[n, idx[n, i, k]]`` the
    k-th neighbour of ``p1[n, i]`` (equal distances by ascending index), both zero in the slots ``k >= lengths2[n]`` and in the rows
    ``i >= lengths1[n]``; ``knn`` = ``knn_gather(p2, idx, lengths2)`` [N, P1, K, D] when ``return_nn``, else None.  ``dists`` is
    differentiable once with respect to both clouds."""
    if p1.dim() != 3 or p2.dim() != 3:
        raise ValueError(f"knn_points: p1 and p2 must be [N, P, D], got {list(p1.shape)} and {list(p2.shape)}")
    N, P1, D = p1.shape
    if p2.shape[0] != N:
        raise ValueError(f"knn_points: p1 has batch dimension {N}, p2 has {p2.shape[0]}")
    if p2.shape[2] != D:
        raise ValueError(f"knn_points: p1 has point dimension {D}, p2 has {p2.shape[2]}")
    if norm not in (1, 2):
        raise ValueError(f"knn_points: norm = {norm!r}, only 1 or 2 norm")

    def lengths_of(given, P):
        return torch.full((N,), P, dtype=torch.int64, device=p1.device) if given is None else given.contiguous()

    dists, idx = _knn_points.apply(p1.contiguous(), p2.contiguous(), lengths_of(lengths1, P1), lengths_of(lengths2, p2.shape[1]), K, norm)
    return _KNN(dists, idx, knn_gather(p2, idx, lengths2) if return_nn else None)


def knn_gather(x: torch.Tensor, idx: torch.Tensor, lengths: Union[torch.Tensor, None] = None):
    """Rows of ``x`` [N, M, U] picked by the ``idx`` [N, L, K] of ``knn_points`` -> [N, L, K, U] with ``out[n, l, k] = x[n, idx[n, l, k]]``,
    and zero in the slots ``k >= lengths[n]`` (``lengths`` int64 [N]: the valid points per cloud of ``x``; None: M).  ``x`` may be the
    cloud that was searched or any per-point feature of it."""
    if x.dim() != 3 or idx.dim() != 3:
        raise ValueError(f"knn_gather: x must be [N, M, U] and idx [N, L, K], got {list(x.shape)} and {list(idx.shape)}")
    N, M, U = x.shape
    L, K = idx.shape[1:]
    if idx.shape[0] != N:
        raise ValueError(f"knn_gather: x has batch dimension {N}, idx has {idx.shape[0]}")
    if M == 0:
        return x.new_zeros((N, L, K, U))
    picked = x[torch.arange(N, device=x.device)[:, None, None], idx]                           # [N, L, K, U]
    # the padding slots hold index 0, not a neighbour; masked always (asking whether any cloud is that short would be a host sync)
    valid = M if lengths is None else lengths.to(x.device)[:, None, None, None]
    slot = torch.arange(K, device=x.device)[None, None, :, None]
    return torch.where(slot < valid, picked, x.new_zeros(()))
