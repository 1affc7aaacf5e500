"""nr3d_lib_amd.bindings._permuto -- drop-in for the reference pybind module ``nr3d_lib.bindings._permuto``
(csrc/permuto/src/permuto.cpp:30-75), backed by the HIP kernels of csrc/permuto*.hip through include/nr3d_hip.h.

Same Python-visible names, argument order / defaults and return structure:
  PermutoEncMeta, permuto_enc_fwd, permuto_enc_bwd, permuto_enc_bwd_bwd_input, supported_n_input_dims.

Deliberate differences:
  * the forward's output is stored feature-major ([E, N]) and returned as a transposed [N, E] view (the fused decoder reads it
    in place, bindings/_mlp.py:_layout); dL_dy may come in either layout;
  * fp16 tables: y and dL/d(dL_dy) are fp32 sums rounded once to half, dL/dparam is accumulated in fp32 and rounded once (the
    reference accumulates in half);
  * ``max_pos_dims`` of ``permuto_enc_bwd`` defaults to None (all dimensions) instead of being required;
  * more argument checks than the reference, all before any launch: every tensor on the positions' device, the table storage
    aligned to the pseudo width, batch offsets multiples of it with a whole table set inside ``lattice_values`` (one
    device-to-host read per call that passes ``batch_offsets``), no more batches of ``batch_data_size`` than table sets.
"""
import ctypes as C

import torch

from .. import _hip as H

MAX_LEVELS, MAX_PSEUDO = 24, 512

# csrc/permuto/src/permuto_cuda.cu:44 (the library's own list, nr3d_permuto_supported_n_input_dims, is checked against it by
# tests/test_permuto_cpu.py; kept here so that the module imports without loading the library)
supported_n_input_dims = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 24, 28, 32, 36, 40, 48, 56, 64]


class _CMeta(C.Structure):
    """nr3d_permuto_meta_t"""
    _fields_ = [
        ("level_scales0", C.c_double * MAX_LEVELS),
        ("level_n_feats", C.c_uint32 * MAX_LEVELS),
        ("level_n_params", C.c_uint32 * MAX_LEVELS),
        ("level_offsets", C.c_uint32 * (MAX_LEVELS + 1)),
        ("level_sizes", C.c_uint32 * MAX_LEVELS),
        ("level_cols", C.c_uint32 * MAX_LEVELS),
        ("map_levels", C.c_uint16 * MAX_PSEUDO),
        ("map_cnt", C.c_uint16 * MAX_PSEUDO),
        ("n_levels", C.c_uint32),
        ("n_pseudo_levels", C.c_uint32),
        ("n_feat_per_pseudo_lvl", C.c_uint32),
        ("n_dims_to_encode", C.c_uint32),
        ("n_encoded_dims", C.c_uint32),
        ("n_params", C.c_uint32),
    ]


class PermutoEncMeta:
    """PermutoEncMeta(n_input_dim, hashmap_size, res_list, n_feats_list) (permuto.h:87-127, create_meta permuto_cuda.cu:46-150).
    Read-only attributes as the reference's def_readonly list (permuto.cpp:58-72)."""

    def __init__(self, n_input_dim: int, hashmap_size: int, res_list, n_feats_list):
        res = [float(r) for r in res_list]
        nf = [int(f) for f in n_feats_list]
        if len(res) != len(nf):
            raise RuntimeError("PermutoEncImpl: Expect `res_list` and `n_feats_list` to have the same length")
        L, D = len(res), int(n_input_dim)
        c = _CMeta()
        scales = (C.c_float * max(L * max(D, 1), 1))()
        H.check(H.lib().nr3d_permuto_meta_create(D, int(hashmap_size), L, (C.c_double * max(L, 1))(*res),
                                                  (C.c_int32 * max(L, 1))(*nf), C.byref(c), scales))
        self._c = c
        self._dev = {}
        self.n_levels = int(c.n_levels)
        self.n_pseudo_levels = int(c.n_pseudo_levels)
        self.n_feat_per_pseudo_lvl = int(c.n_feat_per_pseudo_lvl)
        self.n_dims_to_encode = int(c.n_dims_to_encode)
        self.n_encoded_dims = int(c.n_encoded_dims)
        self.n_params = int(c.n_params)
        self.level_scales0 = [float(v) for v in c.level_scales0[:L]]
        self.level_n_feats = [int(v) for v in c.level_n_feats[:L]]
        self.level_n_params = [int(v) for v in c.level_n_params[:L]]
        self.level_offsets = [int(v) for v in c.level_offsets[:L + 1]]
        self.level_sizes = [int(v) for v in c.level_sizes[:L]]
        self.map_levels = [int(v) for v in c.map_levels[:self.n_pseudo_levels]]
        self.map_cnt = [int(v) for v in c.map_cnt[:self.n_pseudo_levels]]
        self.level_scales_multidim = torch.tensor(list(scales[:L * D]), dtype=torch.float32).view(L, D)

    def _scales(self, device):
        """device copy of level_scales_multidim (uploaded once per device; the reference copies it at every call)"""
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = self.level_scales_multidim.to(device)
        return t

    def __repr__(self):
        return (f"PermutoEncMeta(n_dims_to_encode={self.n_dims_to_encode}, n_levels={self.n_levels}, "
                f"n_encoded_dims={self.n_encoded_dims}, n_params={self.n_params})")


def _rows(t2):
    """[n, w] -> (tensor, row stride, feature stride) the kernels read in place: row-major or feature-major, else a copy"""
    n, w = t2.shape
    if w == 1 or t2.stride(1) == 1:
        return t2, (t2.stride(0) if n > 1 else w), 1
    if n > 1 and t2.stride(0) == 1:
        return t2, 1, t2.stride(1)
    t2 = t2.contiguous()
    return t2, w, 1


def _pcode(params):
    if params.dtype == torch.float32:
        return H.F32
    if params.dtype == torch.float16:
        return H.F16
    raise RuntimeError(f"PermutoEncImpl: lattice_values must be float32 or float16, got {params.dtype}")


def _on_device(fn, dev, **tensors):
    """every tensor argument the kernels read through a raw pointer must live on `dev` (the reference's checkSameGPU,
    permuto_cuda.cu:167-223): a CPU tensor or one on another GPU would reach the kernels as a foreign address"""
    for name, t in tensors.items():
        if t is None:
            continue
        H.require_gpu(t)
        if t.device != dev:
            raise RuntimeError(f"PermutoEncImpl::{fn}: `{name}` is on {t.device}, positions on {dev}")


def _common(fn, meta, positions, params, level_random_shifts, batch_inds, batch_offsets, batch_data_size):
    """the reference's argument checks (permuto_cuda.cu:167-223) -> (N, x, shifts, bidx, boffs, batch_data_size)"""
    H.require_gpu(positions, params)
    _on_device(fn, positions.device, lattice_values=params, batch_inds=batch_inds, batch_offsets=batch_offsets)
    if positions.dim() != 2 or params.dim() != 1:
        raise RuntimeError(f"PermutoEncImpl::{fn}: expected positions [N, D] and 1-D lattice_values")
    if positions.shape[1] != meta.n_dims_to_encode:
        raise RuntimeError(f"PermutoEncImpl::{fn}: positions has {positions.shape[1]} dims, the meta encodes {meta.n_dims_to_encode}")
    if positions.dtype != torch.float32:
        raise RuntimeError("PermutoEncImpl: Input type combination not supported. Supported types are: "
                           "<positions,lattice_values> -> (float, half), (float, float)")
    if positions.device != params.device:
        raise RuntimeError(f"PermutoEncImpl::{fn}: positions and lattice_values are on different devices")
    _pcode(params)
    N = positions.shape[0]
    if params.numel() % meta.n_params != 0:
        raise RuntimeError(f"PermutoEncImpl::{fn}: Expect size of `params`={params.numel()} to be an integral multiple of "
                           f"`n_param`={meta.n_params}")
    shifts = None
    if level_random_shifts is not None:
        if tuple(level_random_shifts.shape) != (meta.n_levels, meta.n_dims_to_encode):
            raise RuntimeError(f"PermutoEncImpl::{fn}: level_random_shifts must be [{meta.n_levels}, {meta.n_dims_to_encode}]")
        shifts = level_random_shifts.detach().to(device=positions.device, dtype=torch.float32).contiguous()
    bidx = None
    if batch_inds is not None:
        if batch_inds.dim() != 1 or batch_inds.shape[0] != N or batch_inds.dtype != torch.long:
            raise RuntimeError(f"PermutoEncImpl::{fn}: batch_inds must be int64 [{N}]")
        bidx = batch_inds.contiguous()
    boffs = None
    if batch_offsets is not None:
        if batch_offsets.dim() != 1 or batch_offsets.dtype != torch.long:
            raise RuntimeError(f"PermutoEncImpl::{fn}: batch_offsets must be 1-D int64")
        boffs = batch_offsets.contiguous()
    bds = 0 if batch_data_size is None else int(batch_data_size)
    if bds != 0 and N % bds != 0:
        raise RuntimeError(f"PermutoEncImpl::{fn}: Expect nonzero `batch_data_size`={bds} to be a divisor of `batch_size`={N}")
    # the kernels read and scatter the tables in vectors of n_feat_per_pseudo_lvl elements: every table set must start on such a
    # boundary (the storage itself, and each batch offset), and lie inside `params`
    pw = meta.n_feat_per_pseudo_lvl
    if params.data_ptr() % (params.element_size() * pw) != 0:
        raise RuntimeError(f"PermutoEncImpl::{fn}: lattice_values storage is not aligned to {pw} elements")
    n_sets = params.numel() // meta.n_params
    if bds and bidx is None and N // bds > (n_sets if boffs is None else boffs.numel()):
        raise RuntimeError(f"PermutoEncImpl::{fn}: {N // bds} batches of `batch_data_size`={bds}, but only "
                           f"{n_sets if boffs is None else boffs.numel()} table sets")
    if boffs is not None and boffs.numel() and bool(((boffs % pw) != 0).logical_or(boffs < 0).logical_or(
            boffs > params.numel() - meta.n_params).any()):
        raise RuntimeError(f"PermutoEncImpl::{fn}: every batch offset must be a multiple of n_feat_per_pseudo_lvl={pw} with a "
                           f"whole table set ({meta.n_params} elements) inside lattice_values ({params.numel()})")
    return N, positions.detach().contiguous(), shifts, bidx, boffs, bds


def permuto_enc_fwd(meta, positions, lattice_values, level_random_shifts=None, batch_inds=None, batch_offsets=None,
                    batch_data_size=None, max_level=None):
    """-> encoded [N, n_encoded_dims] (lattice dtype; a feature-major view)  (permuto_cuda.cu:152-235)"""
    N, x, shifts, bidx, boffs, bds = _common("fwd", meta, positions, lattice_values, level_random_shifts, batch_inds, batch_offsets,
                                             batch_data_size)
    E, dev = meta.n_encoded_dims, positions.device
    max_level = meta.n_levels if max_level is None else int(max_level)
    if max_level <= -1 or N == 0:
        return torch.zeros((N, E), dtype=lattice_values.dtype, device=dev)
    p = lattice_values.detach().contiguous()
    y = H.empty((E, N), dtype=p.dtype, device=dev).t()
    with H.on_device(dev):
        H.check(H.lib().nr3d_permuto_fwd(
            C.byref(meta._c), N, _pcode(p), H.ptr(x), H.ptr(p), H.ptr(meta._scales(dev)), H.ptr(shifts), H.ptr(bidx), H.ptr(boffs),
            bds, max_level, H.ptr(y), y.stride(0), y.stride(1), H.stream_of(x)))
    return y


def _dLdy(meta, dL_dy, N, params):
    _on_device("bwd", params.device, dL_dy=dL_dy)
    if dL_dy.dim() != 2 or tuple(dL_dy.shape) != (N, meta.n_encoded_dims):
        raise RuntimeError(f"PermutoEncImpl: dL_dy must be [{N}, {meta.n_encoded_dims}], got {list(dL_dy.shape)}")
    # dL_dy is read in the lattice dtype (the reference requires the same dtype, permuto_cuda.cu:259)
    return _rows(dL_dy.detach().to(params.dtype))


def permuto_enc_bwd(meta, dL_dy, positions, lattice_values, level_random_shifts=None, batch_inds=None, batch_offsets=None,
                    batch_data_size=None, max_level=None, max_pos_dims=None, need_input_grad=None, need_param_grad=None):
    """-> (dL_dx [N, D] float | None, dL_dparam (lattice dtype) | None)  (permuto_cuda.cu:237-355)"""
    N, x, shifts, bidx, boffs, bds = _common("bwd", meta, positions, lattice_values, level_random_shifts, batch_inds, batch_offsets,
                                             batch_data_size)
    D, dev = meta.n_dims_to_encode, positions.device
    max_level = meta.n_levels if max_level is None else int(max_level)
    max_pos_dims = D if max_pos_dims is None else min(int(max_pos_dims), D)
    need_input_grad = bool(positions.requires_grad) if need_input_grad is None else bool(need_input_grad)
    need_param_grad = bool(lattice_values.requires_grad) if need_param_grad is None else bool(need_param_grad)
    if max_level <= -1 or (not need_input_grad and not need_param_grad):
        return None, None
    g, gsn, gse = _dLdy(meta, dL_dy, N, lattice_values)
    p = lattice_values.detach().contiguous()
    dx = H.empty((N, D), dtype=torch.float32, device=dev) if need_input_grad else None
    dp = torch.zeros(p.numel(), dtype=torch.float32, device=dev) if need_param_grad else None
    if N:
        with H.on_device(dev):
            H.check(H.lib().nr3d_permuto_bwd(
                C.byref(meta._c), N, _pcode(p), H.ptr(g), gsn, gse, H.ptr(x), H.ptr(p), H.ptr(meta._scales(dev)), H.ptr(shifts),
                H.ptr(bidx), H.ptr(boffs), bds, max_level, max_pos_dims, H.ptr(dx), H.ptr(dp), H.stream_of(x)))
    if dp is not None and dp.dtype != p.dtype:
        dp = dp.to(p.dtype)             # fp32 accumulation, one rounding to the table dtype
    return dx, dp


def permuto_enc_bwd_bwd_input(meta, dL_ddLdx, dL_dy, positions, lattice_values, level_random_shifts=None, batch_inds=None,
                              batch_offsets=None, batch_data_size=None, max_level=None, need_dL_ddLdy=None, need_dL_dparams=None):
    """-> (dL_ddLdy [N, E] (lattice dtype) | None, dL_dparam (lattice dtype) | None)  (permuto_cuda.cu:357-526)"""
    N, x, shifts, bidx, boffs, bds = _common("bwdbwd", meta, positions, lattice_values, level_random_shifts, batch_inds,
                                             batch_offsets, batch_data_size)
    D, E, dev = meta.n_dims_to_encode, meta.n_encoded_dims, positions.device
    _on_device("bwdbwd", dev, dL_ddLdx=dL_ddLdx)
    if dL_ddLdx.dim() != 2 or tuple(dL_ddLdx.shape) != (N, D):
        raise RuntimeError(f"PermutoEncImpl::bwdbwd: dL_ddLdx must be [{N}, {D}]")
    max_level = meta.n_levels if max_level is None else int(max_level)
    need_dL_ddLdy = bool(dL_dy.requires_grad) if need_dL_ddLdy is None else bool(need_dL_ddLdy)
    need_dL_dparams = bool(lattice_values.requires_grad) if need_dL_dparams is None else bool(need_dL_dparams)
    if max_level <= -1 or (not need_dL_ddLdy and not need_dL_dparams):
        return None, None
    g, gsn, gse = _dLdy(meta, dL_dy, N, lattice_values)
    gg = dL_ddLdx.detach().to(torch.float32).contiguous()
    p = lattice_values.detach().contiguous()
    ddy = H.empty((N, E), dtype=p.dtype, device=dev) if need_dL_ddLdy else None
    dp = torch.zeros(p.numel(), dtype=torch.float32, device=dev) if need_dL_dparams else None
    if N:
        with H.on_device(dev):
            H.check(H.lib().nr3d_permuto_bwd_bwd_input(
                C.byref(meta._c), N, _pcode(p), H.ptr(gg), H.ptr(g), gsn, gse, H.ptr(x), H.ptr(p), H.ptr(meta._scales(dev)),
                H.ptr(shifts), H.ptr(bidx), H.ptr(boffs), bds, max_level, H.ptr(ddy), E, 1, H.ptr(dp), H.stream_of(x)))
    if dp is not None and dp.dtype != p.dtype:
        dp = dp.to(p.dtype)
    return ddy, dp
