"""Restatement of the reference's permutohedral encoder (csrc/permuto/src/permuto_cuda.cu:46-150, permuto_cuda.h:124-1030) in
torch on the CPU, for the parity tests of csrc/permuto*.hip.

The integer decisions -- elevation, nearest remainder-0 point, ranks, `sum` correction, vertex keys, hash -- are made in float32
torch ops in the kernels' order (both sides round every operation once: the kernels build with -ffp-contract=off), so a point
lands in the same simplex on both.  The barycentric weights and the interpolation are computed in float64 from those float32
elevated values; the elevated values carry the gradient of the linear elevation map, so autograd through this restatement
gives the reference's dL/dx, dL/dparam and the second-order terms of its double backward."""
import math

import torch

SUPPORTED = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 24, 28, 32, 36, 40, 48, 56, 64]


def create_meta(n_input_dim, hashmap_size, res_list, n_feats_list):
    """PermutoEncMeta::create_meta (permuto_cuda.cu:46-150) -> dict, or RuntimeError as the reference"""
    if len(res_list) != len(n_feats_list):
        raise RuntimeError("PermutoEncImpl: Expect `res_list` and `n_feats_list` to have the same length")
    if n_input_dim not in SUPPORTED:
        raise RuntimeError(f"PermutoEncImpl: Currently not supported n_dims_to_encode={n_input_dim}")
    L = len(res_list)
    if L > 24:
        raise RuntimeError(f"PermutoEncImpl: num_level={L} exceeds maximum level=24")
    if all(f % 4 == 0 for f in n_feats_list):
        pw = 4
    elif all(f % 2 == 0 for f in n_feats_list):
        pw = 2
    else:
        raise RuntimeError("PermutoEncImpl: the greatest common divisor of `n_feats_list` must be at least 2")
    scales, offsets, n_params_l, acc, accf = [], [], [], 0, 0.0
    for res, nf in zip(res_list, n_feats_list):
        scales.append([float(torch.tensor(res / math.sqrt(float(d + 1) * (d + 2)), dtype=torch.float32)) for d in range(n_input_dim)])
        accf += float(hashmap_size) * nf
        if accf > float((2 ** 32 - 1) // 2):
            raise RuntimeError("PermutoEncImpl: param size too large.")
        offsets.append(acc)
        n_params_l.append(hashmap_size * nf)
        acc += hashmap_size * nf
    offsets.append(acc)
    map_levels, map_cnt = [], []
    for l, nf in enumerate(n_feats_list):
        for j in range(nf // pw):
            map_levels.append(l)
            map_cnt.append(j)
    return dict(n_dims_to_encode=n_input_dim, n_levels=L, n_feat_per_pseudo_lvl=pw, n_pseudo_levels=len(map_levels),
                n_encoded_dims=sum(n_feats_list), n_params=acc, level_offsets=offsets, level_n_params=n_params_l,
                level_sizes=[hashmap_size] * L, level_n_feats=list(n_feats_list), level_scales0=[float(r) for r in res_list],
                level_scales_multidim=scales, map_levels=map_levels, map_cnt=map_cnt)


def simplex(x32, sc32, sh32):
    """float32 x [N, D], scales [D], shifts [D] | None -> (elevated float32 [N, D+1], rem0 int64, rank int64)
    (permuto_cuda.h:203-264, op for op)"""
    N, D = x32.shape
    elev = [None] * (D + 1)
    sm = torch.zeros(N, dtype=torch.float32)
    for dim in range(D, 0, -1):
        p = x32[:, dim - 1] + (sh32[dim - 1] if sh32 is not None else torch.tensor(0., dtype=torch.float32))
        cf = p * sc32[dim - 1]
        elev[dim] = sm - cf * torch.tensor(float(dim), dtype=torch.float32)
        sm = sm + cf
    elev[0] = sm
    elev = torch.stack(elev, 1)
    v = elev / torch.tensor(float(D + 1), dtype=torch.float32)
    down = torch.floor(v).to(torch.int64) * (D + 1)
    up = down + (D + 1)
    rem0 = torch.where(up.to(torch.float32) - elev < elev - down.to(torch.float32), up, down)
    s = torch.div(rem0.sum(1), D + 1, rounding_mode='trunc')
    rank = torch.zeros(N, D + 1, dtype=torch.int64)
    diff = elev - rem0.to(torch.float32)
    for dim in range(D):
        for o in range(dim + 1, D + 1):
            c = diff[:, dim] < diff[:, o]
            rank[:, dim] += c.long()
            rank[:, o] += (~c).long()
    rank = rank + s[:, None]
    lo, hi = rank < 0, rank > D
    rank = torch.where(lo, rank + D + 1, torch.where(hi, rank - D - 1, rank))
    rem0 = torch.where(lo, rem0 + D + 1, torch.where(hi, rem0 - D - 1, rem0))
    return elev, rem0, rank


def rows(rem0, rank, size):
    """[N, D+1] table rows of the D+1 vertices (key, hash in uint32, % size; permuto_cuda.h:103-121, :300-311)"""
    N, D1 = rank.shape
    D = D1 - 1
    M = 0xFFFFFFFF
    out = []
    for k in range(D + 1):
        h = torch.zeros(N, dtype=torch.int64)
        for dim in range(D):
            key = rem0[:, dim] + k - (D + 1) * (rank[:, dim] > D - k).long()
            h = (h + key) & M
            h = (h * 2531011) & M
        out.append(h % size)
    return torch.stack(out, 1)


def encode(meta, x32, params, scales=None, shifts=None, bidx=None, boffs=None, bds=0, max_level=None, x64=None):
    """y float64 [N, n_encoded_dims].  params: float64 1-D (may require grad); x64: float64 [N, D] that requires grad, whose values
    equal x32 (the gradient path for dL/dx; the simplex decisions always come from x32)"""
    N, D = x32.shape
    L = meta['n_levels']
    scales = torch.tensor(meta['level_scales_multidim'], dtype=torch.float32) if scales is None else scales.float().cpu()
    max_level = L if max_level is None else max_level
    if bidx is not None:
        b = bidx.cpu().long()
        live = b >= 0
        b = b.clamp(min=0)
    else:
        b = (torch.arange(N) // bds) if bds else torch.zeros(N, dtype=torch.int64)
        live = torch.ones(N, dtype=torch.bool)
    base = boffs.cpu().long()[b] if boffs is not None else b * meta['n_params']
    cols = []
    for l in range(L):
        nf, size, off = meta['level_n_feats'][l], meta['level_sizes'][l], meta['level_offsets'][l]
        if l > max_level:
            cols.append(torch.zeros(N, nf, dtype=torch.float64))
            continue
        sc = scales[l]
        sh = shifts[l].float().cpu() if shifts is not None else None
        elev32, rem0, rank = simplex(x32, sc, sh)
        elev = elev32.double()
        if x64 is not None:                       # straight-through: values of elev32, gradient of the linear elevation map
            xs = x64 * sc.double()
            csum = torch.flip(torch.cumsum(torch.flip(xs, [1]), 1), [1])      # sum_{j >= d} xs[j]
            lin = torch.cat([csum[:, :1], csum[:, 1:] - torch.arange(1, D, dtype=torch.float64) * xs[:, :-1],
                             -float(D) * xs[:, -1:]], 1)
            elev = elev + (lin - lin.detach())
        delta = (elev - rem0.double()) / (D + 1)
        bary = torch.zeros(N, D + 2, dtype=torch.float64)
        bary = bary.scatter_add(1, D - rank, delta).scatter_add(1, D + 1 - rank, -delta)
        w = torch.cat([bary[:, :1] + 1.0 + bary[:, D + 1:D + 2], bary[:, 1:D + 1]], 1)
        r = rows(rem0, rank, size)
        idx = (base + off)[:, None, None] + r[:, :, None] * nf + torch.arange(nf)[None, None, :]
        vals = params[idx.reshape(-1)].view(N, D + 1, nf)
        y = (w[:, :, None] * vals).sum(1)
        cols.append(torch.where(live[:, None], y, torch.zeros_like(y)))
    return torch.cat(cols, 1)
