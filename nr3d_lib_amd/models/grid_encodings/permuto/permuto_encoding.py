"""``PermutoEncoding``: the permutohedral-lattice encoder module a field holds -- owns the fp32 ``flattened_params`` (its
checkpoint format) and feeds them to the HIP-backed ``PermutoEncImpl``.

Counterpart of nr3d_lib/models/grid_encodings/permuto/permuto_encoding.py, modelled on ``LoTDEncoding``: constructor keywords,
``forward`` / ``backward_dydx`` (with a space, inputs in [-1, 1] are mapped to [0, 1] and the nablas halved), ``space_cfg`` of
type 'aabb' / 'batched' / 'unbounded', the 'uniform' / 'normal' ``param_init_cfg``, ``max_level`` / ``window`` masking driven by
``anneal_cfg`` (``MultiresAnnealer``, ``set_anneal_iter``), ``get_level_param`` / ``set_level_param``, ``inference_param``,
``clip_grad_and_update_ema``, ``stat_param`` and the ``permuto_cfg`` extra state.  Not provided (as for ``LoTDEncoding``): the
'aabb_dynamic' / 'batched_dynamic' spaces and ``permuto_auto_compute_cfg``'s ``stretch`` (the reference's ``get_permuto_cfg``
ignores it too)."""
from copy import deepcopy
from math import prod
from typing import Any, Dict, Optional, Union

import torch
import torch.nn as nn

from .permuto import PermutoEncImpl, get_permuto_cfg, level_param_index_shape

__all__ = ['PermutoEncoding']


def _as_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        return dtype
    return {'half': torch.half, 'float16': torch.half, 'float': torch.float, 'float32': torch.float}[str(dtype)]


class PermutoEncoding(nn.Module):
    def __init__(self, input_ch: int, *, permuto_cfg: dict = None, permuto_auto_compute_cfg: dict = None,
                 pos_scale: Union[float, torch.Tensor] = None, space: nn.Module = None, space_cfg: dict = None,
                 anneal_cfg: dict = None, param_init_cfg={'type': 'uniform', 'bound': 1.0e-4},
                 clip_level_grad_ema_factor: float = 0, dtype=torch.half, device=None) -> None:
        super().__init__()
        self.dtype = _as_dtype(dtype)
        self.clip_level_grad_ema_factor = clip_level_grad_ema_factor
        self.param_init_cfg = param_init_cfg
        if space is None and space_cfg is not None:
            space_cfg = dict(space_cfg)
            space_type = space_cfg.pop('type').lower()
            if space_type == 'aabb':
                from nr3d_lib_amd.models.spatial import AABBSpace
                space = AABBSpace(**space_cfg)
            elif space_type == 'batched':
                from nr3d_lib_amd.models.spatial import BatchedBlockSpace
                space = BatchedBlockSpace(**space_cfg)
            elif space_type in ('unbounded', 'none'):
                space = None
            else:
                raise RuntimeError(f"Invalid space_type={space_type}")
        self.space = space
        assert (permuto_cfg is not None) != (permuto_auto_compute_cfg is not None), \
            "Please specify one and only one of `permuto_cfg` and `permuto_auto_compute_cfg`"
        if permuto_auto_compute_cfg is not None:
            permuto_cfg = get_permuto_cfg(**permuto_auto_compute_cfg, input_ch=input_ch)
        else:
            permuto_cfg = deepcopy(permuto_cfg if isinstance(permuto_cfg, dict) else permuto_cfg.to_dict())
        if pos_scale is not None:
            permuto_cfg.update(pos_scale=pos_scale)
        self.permuto_cfg = permuto_cfg
        self.permuto = PermutoEncImpl(input_ch, **permuto_cfg, dtype=self.dtype, device=device)
        self.in_features: int = input_ch
        self.out_features: int = self.permuto.out_features
        # parameters are always stored in fp32; `dtype` only decides what the kernels are fed
        self.flattened_params = nn.Parameter(torch.zeros(self.permuto.n_params, device=device, dtype=torch.float))
        self.init_lattice_values_random()
        self.annealer = None
        if anneal_cfg is not None:
            from ..multires_annealer import MultiresAnnealer
            self.annealer = MultiresAnnealer(self.permuto.level_n_feats, **anneal_cfg, dtype=self.dtype, device=device)
        self.window: Optional[torch.Tensor] = None      # optional soft mask on the output features
        self.max_level: Optional[int] = None            # levels above it are skipped (-1: all of them)
        if clip_level_grad_ema_factor > 0:
            self.register_buffer("level_grad_norm_ema", torch.full([self.permuto.n_levels], 0.1, device=device))

    device = property(lambda self: self.flattened_params.device)
    level_n_feats = property(lambda self: self.permuto.level_n_feats)
    meta = property(lambda self: self.permuto.meta)
    inference_param = property(lambda self: self.flattened_params.data.to(self.dtype))

    def set_anneal_iter(self, cur_it: int):
        if self.annealer is not None:
            self.max_level, self.window = self.annealer(cur_it)

    def forward(self, input: torch.Tensor, max_level: int = None, need_dL_dinput: Optional[bool] = None) -> torch.Tensor:
        """features at ``input`` (in [-1, 1] when the encoder has a space) -> [..., out_features]"""
        if self.space is not None:
            input = input / 2. + 0.5
        out = self.permuto.forward(input, self.flattened_params, max_level=(max_level or self.max_level),
                                   need_dL_dinput=need_dL_dinput)
        return (out * self.window) if self.window is not None else out

    def backward_dydx(self, dL_dy: torch.Tensor, input: torch.Tensor, max_level: int = None,
                      max_pos_dims: int = None) -> torch.Tensor:
        """nablas dL/d(input) from dL/dy (differentiable once more into dL_dy and the lattice: second order)"""
        if self.space is not None:
            return self.permuto.backward_dydx(dL_dy, input / 2. + 0.5, self.flattened_params,
                                              max_level=(max_level or self.max_level), max_pos_dims=max_pos_dims) / 2.
        return self.permuto.backward_dydx(dL_dy, input, self.flattened_params, max_level=(max_level or self.max_level),
                                          max_pos_dims=max_pos_dims)

    def get_level_param(self, l: int, grad=False) -> torch.Tensor:
        index, shape = level_param_index_shape(self.meta, l)
        return (self.flattened_params.grad if grad else self.flattened_params)[index].view(shape)

    def set_level_param(self, l: int, value: torch.Tensor = ...):
        index, shape = level_param_index_shape(self.meta, l)
        with torch.no_grad():
            self.flattened_params[index] = value.contiguous().view(prod(shape))

    @torch.no_grad()
    def init_lattice_values_random(self):
        cfg = self.param_init_cfg
        kind = cfg['type']
        if kind == 'uniform':
            self.flattened_params.uniform_(-cfg['bound'], cfg['bound'])
        elif kind == 'normal':
            self.flattened_params.normal_(0, cfg['std'])
        else:
            raise RuntimeError(f"Invalid param_init_method={kind}")

    def get_extra_state(self) -> Any:
        return self.permuto_cfg

    def set_extra_state(self, state: Any):
        self.permuto_cfg = state

    @torch.no_grad()
    def clip_grad_and_update_ema(self, val: float = None):
        """per-level gradient-norm clipping against a running norm (as LoTDEncoding's): the EMA of each level's gradient 2-norm
        moves 1 % towards the current norm, then the level's gradient is rescaled to at most clip_level_grad_ema_factor x that
        EMA.  No-op unless built with clip_level_grad_ema_factor > 0."""
        if not self.clip_level_grad_ema_factor > 0 or self.flattened_params.grad is None:
            return
        L = self.permuto.n_levels
        gnorm = torch.stack([self.get_level_param(l, grad=True).norm() for l in range(L)])
        ema = self.level_grad_norm_ema.copy_(gnorm.lerp(self.level_grad_norm_ema, 0.99))
        for l in range(L):
            g = self.get_level_param(l, grad=True)
            g.mul_((self.clip_level_grad_ema_factor * ema[l] / (gnorm[l] + 1e-6)).clamp(max=1.0))

    @torch.no_grad()
    def stat_param(self, with_grad: bool = False, prefix: str = '') -> Dict[str, float]:
        """mean / std / min / max / absmax / norm of all parameters and of every level, optionally of their gradients"""
        def stats(t: torch.Tensor, key: str):
            t = t.detach().float()
            if t.numel() == 1:
                return {f"{key}.val": t.item(), f"{key}.mean": t.item()}
            return {f"{key}.mean": t.mean().item(), f"{key}.std": t.std().item(), f"{key}.min": t.min().item(),
                    f"{key}.max": t.max().item(), f"{key}.absmax": t.abs().max().item(), f"{key}.norm": t.norm().item()}
        pre = prefix + ('.' if prefix and not prefix.endswith('.') else '')
        with_grad = with_grad and self.flattened_params.grad is not None
        out = stats(self.flattened_params, pre + 'total')
        if with_grad:
            out.update(stats(self.flattened_params.grad, pre + 'grad_total'))
        for l in range(self.permuto.n_levels):
            out.update(stats(self.get_level_param(l), f"{pre}lv.{l}"))
            if with_grad:
                out.update(stats(self.get_level_param(l, grad=True), f"{pre}grad.lv.{l}"))
        return out
