"""nr3d_lib_amd.maths.chamfer_distance -- ``chamfer_distance`` with the name, signature and backends of the reference's
``nr3d_lib.maths.chamfer_distance``, written from that contract: for every point of one cloud the distance to the nearest point of the
other, in both directions.

    'pt3d' (default)  ``maths.pytorch3d_knn.knn_points`` with K = 1, i.e. the HIP k-NN kernel of csrc/knn.hip for GPU tensors;
                      differentiable through its backward
    'pt3d_import'     the same two searches through pytorch3d's own ``knn_points``, imported only when this backend is asked for
    'pytorch'         the minimum over the dense [..., N1, N2] matrix of squared distances (norm 2 only; memory grows with N1 N2)

The reference's dense backend measures x against itself (it builds its second operand from ``x``); here it measures x against y, as its
docstring says.  The reference's unused ``cv2`` import is not repeated."""
from typing import Literal, Tuple

import torch

__all__ = ['chamfer_distance', 'chamfer_distance_pytorch', 'chamfer_distance_pt3d_import', 'chamfer_distance_pt3d_borrowed']


def chamfer_distance(
    x: torch.Tensor, y: torch.Tensor, norm: int = 2,
    backend: Literal['pytorch', 'pt3d_import', 'pt3d'] = 'pt3d') -> Tuple[torch.Tensor, torch.Tensor]:
    """x [(B,) N1, D], y [(B,) N2, D] -> (x_to_y [(B,) N1], y_to_x [(B,) N2]): the distance of every point to its nearest point in the
    other cloud, squared Euclidean for ``norm`` 2, sum of absolute differences for ``norm`` 1.  The batch dimension may be left out."""
    if backend == 'pt3d':
        return chamfer_distance_pt3d_borrowed(x, y, norm=norm)
    if backend == 'pt3d_import':
        return chamfer_distance_pt3d_import(x, y, norm=norm)
    if backend == 'pytorch':
        assert norm == 2, f"chamfer_distance: the 'pytorch' backend has norm 2 only, got norm {norm}"
        return chamfer_distance_pytorch(x, y)
    raise RuntimeError(f"chamfer_distance: unknown backend {backend!r}, one of 'pt3d', 'pt3d_import', 'pytorch'")


def chamfer_distance_pytorch(x: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Both directions from one dense matrix of squared distances: rows are points of x, columns points of y.  For small clouds only."""
    assert x.dim() >= 2 and x.dim() == y.dim() and x.shape[-1] == y.shape[-1], \
        f"chamfer_distance: x {list(x.shape)} and y {list(y.shape)} must agree in rank and point dimension"
    sq = (x[..., :, None, :] - y[..., None, :, :]).square().sum(-1)
    return sq.min(dim=-1).values, sq.min(dim=-2).values


def _nearest_both_ways(search, x, y, norm):
    """``search`` is a ``knn_points``; unbatched clouds get a batch dimension for the search and lose it again"""
    if norm not in (1, 2):
        raise ValueError(f"chamfer_distance: norm = {norm!r}, only 1 or 2 norm")
    xb, yb = (c.unsqueeze(0) if c.dim() == 2 else c for c in (x, y))
    if xb.dim() != 3 or yb.dim() != 3 or xb.shape[0] != yb.shape[0] or xb.shape[2] != yb.shape[2]:
        raise ValueError(f"chamfer_distance: x {list(x.shape)} and y {list(y.shape)} must agree in batch and point dimensions")
    x_to_y = search(xb, yb, norm=norm, K=1).dists.squeeze(-1)
    y_to_x = search(yb, xb, norm=norm, K=1).dists.squeeze(-1)
    return (x_to_y[0] if x.dim() == 2 else x_to_y), (y_to_x[0] if y.dim() == 2 else y_to_x)


def chamfer_distance_pt3d_import(x: torch.Tensor, y: torch.Tensor, norm: int = 2) -> Tuple[torch.Tensor, torch.Tensor]:
    from pytorch3d.ops.knn import knn_points
    return _nearest_both_ways(knn_points, x, y, norm)


def chamfer_distance_pt3d_borrowed(x: torch.Tensor, y: torch.Tensor, norm: int = 2) -> Tuple[torch.Tensor, torch.Tensor]:
    from .pytorch3d_knn import knn_points
    return _nearest_both_ways(knn_points, x, y, norm)
