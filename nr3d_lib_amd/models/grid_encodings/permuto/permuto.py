"""Permutohedral-lattice encoding (PermutoSDF's encoding; Rosu & Behnke, CVPR 2023) on the HIP kernels of csrc/permuto*.hip.

Counterpart of nr3d_lib/models/grid_encodings/permuto/permuto.py: ``generate_meta``, ``level_param_index_shape``,
``get_permuto_cfg``, the autograd functions ``PermutoEncFunction`` (y; first-order dL/dx and dL/dparam) and
``PermutoEncBwdInputFunction`` (nablas dL/dx, differentiable once more into dL_dy and the lattice), the functional
``permuto_enc_fwd`` / ``permuto_enc_bwd_input`` and the ``PermutoEncImpl`` module, with the reference's ``loss_scale``
(128 for half tables), ``pos_scale`` (a per-dimension tensor), ``max_level``, ``max_pos_dims`` and batching semantics.
"""
from math import prod
from typing import List, Optional, Union

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

import nr3d_lib_amd.bindings._permuto as _backend

__all__ = [
    'generate_meta',
    'level_param_index_shape',
    'get_permuto_cfg',
    'PermutoEncFunction',
    'PermutoEncBwdInputFunction',
    'permuto_enc_fwd',
    'permuto_enc_bwd_input',
    'PermutoEncImpl',
]


def generate_meta(n_input_dim: int, res_list: List[float], n_feats_list: List[int], hashmap_size: int):
    assert n_input_dim in _backend.supported_n_input_dims, \
        f"n_input_dim={n_input_dim} not in supported list={_backend.supported_n_input_dims}"
    return _backend.PermutoEncMeta(n_input_dim, hashmap_size, res_list, n_feats_list)


def level_param_index_shape(meta, l: int):
    M = meta.level_n_feats[l]
    size = meta.level_sizes[l]
    offset = meta.level_offsets[l]
    offset_next = meta.level_offsets[l + 1]
    index = (slice(offset, offset_next),)
    shape = (size, M)
    return index, shape


def get_permuto_cfg(type: str, input_ch: int = ..., stretch: Union[float, List[float]] = None, **kwargs) -> dict:
    def multi_res_cfg(coarsest_res: float = 10.0, finest_res: float = 1000.0, n_levels: int = 16, n_feats: int = 2,
                      log2_hashmap_size: int = 19, **other_kwargs):
        res_list = np.geomspace(coarsest_res, finest_res, num=n_levels)
        n_feats_list = [n_feats] * n_levels
        hashmap_size = 2 ** log2_hashmap_size
        return dict(res_list=res_list, n_feats_list=n_feats_list, hashmap_size=hashmap_size, **other_kwargs)

    if type == 'multi_res':
        return multi_res_cfg(**kwargs)
    raise RuntimeError(f"Invalid type={type}")


class PermutoEncFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, positions, lattice_values, level_random_shifts=None, bidx=None, batch_offsets=None, batch_data_size=None,
                loss_scale=1.0, pos_scale=1.0, max_level=None, need_dL_dinput: Optional[bool] = None):
        if need_dL_dinput is None:
            need_dL_dinput = torch.is_grad_enabled() and positions.requires_grad
        ctx.set_materialize_grads(False)
        prefix = positions.shape[:-1]
        bidx = None if bidx is None else bidx.contiguous().long().flatten()
        encoded = _backend.permuto_enc_fwd(meta, positions.flatten(0, -2) * pos_scale, lattice_values, level_random_shifts,
                                           bidx, batch_offsets, batch_data_size, max_level)
        if need_dL_dinput or ctx.needs_input_grad[2]:
            ctx.save_for_backward(positions, lattice_values, level_random_shifts, bidx, batch_offsets,
                                  pos_scale if isinstance(pos_scale, torch.Tensor) else None)
            ctx.pos_scale_num = None if isinstance(pos_scale, torch.Tensor) else pos_scale
            ctx.meta = meta
            ctx.prefix = prefix
            ctx.batch_data_size = batch_data_size
            ctx.loss_scale = loss_scale
            ctx.max_level = max_level
            ctx.need_dL_dinput = need_dL_dinput
        return encoded.unflatten(0, prefix)

    @staticmethod
    @once_differentiable
    def backward(ctx, dL_dy):
        dL_dx = dL_dparam = None
        if dL_dy is not None and (ctx.need_dL_dinput or ctx.needs_input_grad[2]):
            positions, lattice_values, level_random_shifts, bidx, batch_offsets, pos_scale = ctx.saved_tensors
            pos_scale = ctx.pos_scale_num if pos_scale is None else pos_scale
            loss_scale = ctx.loss_scale
            dL_dx, dL_dparam = _backend.permuto_enc_bwd(
                ctx.meta, dL_dy.flatten(0, -2) * loss_scale, positions.flatten(0, -2) * pos_scale, lattice_values,
                level_random_shifts, None if bidx is None else bidx.flatten(0, -1), batch_offsets, ctx.batch_data_size,
                ctx.max_level, None, ctx.need_dL_dinput, ctx.needs_input_grad[2])
            dL_dx = None if dL_dx is None else (dL_dx.unflatten(0, ctx.prefix) * (pos_scale / loss_scale))
            dL_dparam = None if dL_dparam is None else (dL_dparam / loss_scale)
        # 0:meta, 1:positions, 2:lattice_values, 3..10
        return None, dL_dx, dL_dparam, None, None, None, None, None, None, None, None


class PermutoEncBwdInputFunction(torch.autograd.Function):
    """nablas dL/dx from dL_dy, with second-order gradients into dL_dy and the lattice (not into x: the reference's limit).
    Use this, not PermutoEncFunction's backward under create_graph, to compute nablas (permuto.py of the reference)."""
    @staticmethod
    def forward(ctx, meta, dL_dy, positions, lattice_values, level_random_shifts, bidx, batch_offsets, batch_data_size,
                loss_scale=1.0, pos_scale=1.0, max_level=None, max_pos_dims=None):
        ctx.set_materialize_grads(False)
        prefix = positions.shape[:-1]
        bidx = None if bidx is None else bidx.contiguous().long().flatten()
        dL_dx, _ = _backend.permuto_enc_bwd(
            meta, dL_dy.flatten(0, -2) * loss_scale, positions.flatten(0, -2) * pos_scale, lattice_values, level_random_shifts,
            bidx, batch_offsets, batch_data_size, max_level, max_pos_dims, True, False)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[3]:
            ctx.save_for_backward(dL_dy, positions, lattice_values, level_random_shifts, bidx, batch_offsets,
                                  pos_scale if isinstance(pos_scale, torch.Tensor) else None)
            ctx.pos_scale_num = None if isinstance(pos_scale, torch.Tensor) else pos_scale
            ctx.meta = meta
            ctx.batch_data_size = batch_data_size
            ctx.loss_scale = loss_scale
            ctx.max_level = max_level
            ctx.max_pos_dims = max_pos_dims
        return None if dL_dx is None else (dL_dx.unflatten(0, prefix) * (pos_scale / loss_scale))

    @staticmethod
    @once_differentiable
    def backward(ctx, dL_ddLdx):
        # second order: d(dL_dx)/d(dL_dy) and d(dL_dx)/d(params); d(dL_dx)/dx is not provided (as in the reference)
        dL_ddLdy = dL_dparam = None
        if dL_ddLdx is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[3]):
            dL_dy, positions, lattice_values, level_random_shifts, bidx, batch_offsets, pos_scale = ctx.saved_tensors
            pos_scale = ctx.pos_scale_num if pos_scale is None else pos_scale
            prefix = positions.shape[:-1]
            loss_scale = ctx.loss_scale
            dL_ddLdy, dL_dparam = _backend.permuto_enc_bwd_bwd_input(
                ctx.meta, dL_ddLdx.flatten(0, -2).to(positions.dtype) * pos_scale, dL_dy.flatten(0, -2) * loss_scale,
                positions.flatten(0, -2) * pos_scale, lattice_values, level_random_shifts,
                None if bidx is None else bidx.flatten(), batch_offsets, ctx.batch_data_size, ctx.max_level,
                ctx.needs_input_grad[1], ctx.needs_input_grad[3])
            dL_ddLdy = None if dL_ddLdy is None else dL_ddLdy.unflatten(0, prefix).to(dL_dy.dtype)
            dL_dparam = None if dL_dparam is None else (dL_dparam / loss_scale)
        # 0:meta, 1:dL_dy, 2:positions, 3:lattice_values, 4..11
        return None, dL_ddLdy, None, dL_dparam, None, None, None, None, None, None, None, None


def permuto_enc_fwd(positions: torch.Tensor, lattice_values: torch.Tensor, level_random_shifts: torch.Tensor = None,
                    bidx: torch.Tensor = None, batch_offsets: torch.Tensor = None, input_batched=False, max_level=None,
                    need_dL_dinput: Optional[bool] = None, pos_scale: float = 1.0, meta=None, n_input_dim: int = None,
                    res_list: List[float] = None, n_feats_list: Union[int, List[int]] = None, hashmap_size: int = None) -> torch.Tensor:
    if need_dL_dinput is None:
        need_dL_dinput = torch.is_grad_enabled() and positions.requires_grad
    if meta is None:
        meta = generate_meta(n_input_dim, res_list, n_feats_list, hashmap_size)
    if input_batched:
        batch_data_size = prod(positions.shape[1:-1])
        bidx = None
    else:
        batch_data_size = 0
    loss_scale = 128.0 if (lattice_values.dtype == torch.float16) else 1.
    return PermutoEncFunction.apply(meta, positions.float(), lattice_values, level_random_shifts, bidx, batch_offsets,
                                    batch_data_size, loss_scale, pos_scale, max_level, need_dL_dinput)


def permuto_enc_bwd_input(meta, dL_dy: torch.Tensor, positions: torch.Tensor, lattice_values: torch.Tensor,
                          level_random_shifts: torch.Tensor = None, bidx: torch.Tensor = None, batch_offsets: torch.Tensor = None,
                          input_batched=False, max_level: int = None, max_pos_dims: int = None, pos_scale: float = 1.0) -> torch.Tensor:
    if input_batched:
        batch_data_size = prod(positions.shape[1:-1])
        bidx = None
    else:
        batch_data_size = 0
    loss_scale = 128.0 if (lattice_values.dtype == torch.float16) else 1.
    return PermutoEncBwdInputFunction.apply(meta, dL_dy, positions.float(), lattice_values, level_random_shifts, bidx,
                                            batch_offsets, batch_data_size, loss_scale, pos_scale, max_level, max_pos_dims)


class PermutoEncImpl(nn.Module):
    def __init__(self, in_features: int, res_list: List[float], n_feats_list: List[int], hashmap_size: int = None,
                 log2_hashmap_size: int = None, apply_random_shifts_per_level=True, pos_scale: float = 1.0, dtype=torch.half,
                 device=None) -> None:
        super().__init__()
        assert dtype == torch.float or dtype == torch.float16, "dtype must be one of torch.float or torch.float16"
        assert bool(log2_hashmap_size is None) != bool(hashmap_size is None), \
            "Please specify one of [hashmap_size, log2_hashmap_size]"
        self.loss_scale = 128.0 if dtype == torch.float16 else 1.0
        self.dtype = dtype
        if log2_hashmap_size is not None:
            hashmap_size = 2 ** log2_hashmap_size
        self.meta = generate_meta(in_features, res_list, n_feats_list, hashmap_size)
        if apply_random_shifts_per_level:
            shifts = 10.0 * torch.randn([self.n_levels, self.in_features], dtype=torch.float, device=device)
        else:
            shifts = torch.zeros([self.n_levels, self.in_features], dtype=torch.float, device=device)
        self.register_buffer('level_random_shifts', shifts, persistent=True)
        pos_scale = torch.as_tensor(pos_scale, dtype=torch.float, device=device).expand(in_features).clone()
        self.register_buffer('pos_scale', pos_scale, persistent=True)
        self.params = {
            'in_features': in_features, 'res_list': res_list, 'n_feats_list': n_feats_list, 'hashmap_size': hashmap_size,
            'log2_hashmap_size': log2_hashmap_size, 'apply_random_shifts_per_level': apply_random_shifts_per_level,
            'pos_scale': pos_scale, 'dtype': dtype, 'device': device,
        }

    in_features = property(lambda self: self.meta.n_dims_to_encode)
    out_features = property(lambda self: self.meta.n_encoded_dims)
    n_levels = property(lambda self: self.meta.n_levels)
    n_params = property(lambda self: self.meta.n_params)
    level_scales0 = property(lambda self: self.meta.level_scales0)
    level_sizes = property(lambda self: self.meta.level_sizes)
    level_offsets = property(lambda self: self.meta.level_offsets)
    level_n_feats = property(lambda self: self.meta.level_n_feats)
    level_n_params = property(lambda self: self.meta.level_n_params)

    def forward(self, positions: torch.Tensor, lattice_values: torch.Tensor, bidx: torch.Tensor = None,
                batch_offsets: torch.Tensor = None, input_batched=False, max_level: int = None,
                need_dL_dinput: Optional[bool] = None) -> torch.Tensor:
        if need_dL_dinput is None:
            need_dL_dinput = torch.is_grad_enabled() and positions.requires_grad
        if input_batched:
            assert bidx is None, 'bidx is only taken care of when input is not batched.'
            batch_data_size = prod(positions.shape[1:-1])
        else:
            batch_data_size = 0
        return PermutoEncFunction.apply(self.meta, positions.float(), lattice_values.to(self.dtype), self.level_random_shifts,
                                        bidx, batch_offsets, batch_data_size, self.loss_scale, self.pos_scale, max_level,
                                        need_dL_dinput)

    def backward_dydx(self, dL_dy: torch.Tensor, positions: torch.Tensor, lattice_values: torch.Tensor, bidx: torch.Tensor = None,
                      batch_offsets: torch.Tensor = None, input_batched=False, max_level: int = None,
                      max_pos_dims: int = None) -> torch.Tensor:
        if input_batched:
            assert bidx is None, 'bidx is only taken care of when input is not batched.'
            batch_data_size = prod(positions.shape[1:-1])
        else:
            batch_data_size = 0
        return PermutoEncBwdInputFunction.apply(self.meta, dL_dy, positions.float(), lattice_values.to(self.dtype),
                                                self.level_random_shifts, bidx, batch_offsets, batch_data_size, self.loss_scale,
                                                self.pos_scale, max_level, max_pos_dims)

    def __getstate__(self):
        self.params['device'] = self.level_random_shifts.device
        self.params['level_random_shifts'] = self.level_random_shifts
        return self.params

    def __setstate__(self, state_dict):
        state_dict = dict(state_dict)
        level_random_shifts = state_dict.pop('level_random_shifts')
        self.__init__(**state_dict)
        self.level_random_shifts = level_random_shifts

    def extra_repr(self) -> str:
        ele_size = {torch.float32: 4, torch.float16: 2}[self.dtype]
        return (f"in_dim={self.meta.n_dims_to_encode}, out_dim={self.meta.n_encoded_dims}, num_levels={self.meta.n_levels}, "
                f"num_params={self.meta.n_params}, params_size={(self.meta.n_params * ele_size) / (1024 ** 2):.3f} MiB, "
                f"dtype={self.dtype}\nlevel_scales0={self.meta.level_scales0}\nlevel_n_feats={self.meta.level_n_feats}")
