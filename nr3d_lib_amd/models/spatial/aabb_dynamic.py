"""Single axis-aligned block of a time-varying scene -- counterpart of ``AABBDynamicSpace``
(nr3d_lib/models/spatial/aabb_dynamic.py:21-38): the box of ``AABBSpace`` plus the (identity) timestamp maps; timestamps live
in [-1, 1]."""
from typing import Tuple

import torch

from .aabb import AABBSpace

__all__ = ['AABBDynamicSpace']


class AABBDynamicSpace(AABBSpace):
    def normalize_ts(self, ts: torch.Tensor):
        return ts

    def unnormalize_ts(self, ts: torch.Tensor):
        return ts

    def sample_pts_uniform(self, num_pts: int) -> Tuple[torch.Tensor, torch.Tensor]:
        x = super().sample_pts_uniform(num_pts)
        ts = torch.empty([num_pts], dtype=torch.float, device=self.device).uniform_(-1, 1)
        return x, ts
