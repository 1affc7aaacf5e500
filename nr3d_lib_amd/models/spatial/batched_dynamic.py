"""A batch of time-varying objects that share one box -- counterpart of ``BatchedDynamicSpace``
(nr3d_lib/models/spatial/batched_dynamic.py:20-41): ``BatchedBlockSpace`` plus the (identity) timestamp maps; the ray test hands
per-ray extras such as ``rays_ts`` [B, N_rays] through to the flat records."""
from typing import Tuple

import torch

from .batched import BatchedBlockSpace

__all__ = ['BatchedDynamicSpace']


class BatchedDynamicSpace(BatchedBlockSpace):
    def cur_batch__normalize_ts(self, ts: torch.Tensor, bidx: torch.LongTensor = None):
        return ts

    def cur_batch__unnormalize_ts(self, ts: torch.Tensor, bidx: torch.LongTensor = None):
        return ts

    def cur_batch__sample_pts_uniform(self, batch_size: int,
                                      num_pts_per_batch: int) -> Tuple[torch.Tensor, torch.LongTensor, torch.Tensor]:
        x, bidx = super().cur_batch__sample_pts_uniform(batch_size, num_pts_per_batch)
        ts = torch.empty([batch_size, num_pts_per_batch], dtype=torch.float, device=self.device).uniform_(-1, 1)
        return x, bidx, ts
