"""Label-carrying restatement of one packed up-sampling stage and of the up-sampling loop of the forest NeuS queries, on top of
tests/neus_packed_ref.py: every sample carries an int64 label (its block index), a new depth takes the label of `pos`, the upper end
of the CDF bin the inversion found (before the running maximum), and the union carries the labels along.  Adds `pos`, `cdf`,
`blidx_fine` and `blidx_merged` to what neus_packed_ref.stage returns.

`pos` is a decision: where u_j meets a CDF knot, float32 and float64 may find neighbouring bins.  proven_ties() marks the cases
(p, j) for which a float64 knot of the pack lies within tau of u_j; tau = 4 x the largest |cdf32 - cdf64| over the inputs at hand
(cdf_tau), computed by the test that uses it.

Also a plain-loop restatement of the linear stepper inside packed segments (graphics.raysample)."""
import numpy as np
import torch

import neus_packed_ref as ref


def pack_cdf(alpha):
    """the normalised exclusive sum of the early-stopped weights of ONE pack: pack_stage's own lines up to the inversion"""
    n = alpha.shape[0]
    keep = torch.where(alpha <= 0, torch.ones_like(alpha), 1.0 - alpha)
    T = torch.cat([torch.ones_like(keep[:1]), ref._cumprod(keep)[:-1]])
    below = (T < ref.EARLY_STOP).nonzero()
    stop = int(below[0]) if below.numel() else n
    w = alpha * T
    w[stop:] = 0
    cdf = torch.cat([torch.zeros_like(w[:1]), ref._cumsum(w)[:-1]])
    return cdf / cdf[-1].clamp_min(ref.MASS_MIN)


def stage(depth, sdf, blidx, pack_infos, u, inv_s, use_estimate, dtype=torch.float32):
    """neus_packed_ref.stage plus: pos int64 [P, m] (inside the pack), cdf [N], blidx_fine int64 [P, m] = blidx[first + pos],
    blidx_merged int64 [N + P m] (old labels at pidx_old, new ones at pidx_fine)"""
    r = ref.stage(depth, sdf, pack_infos, u, inv_s, use_estimate, dtype)
    P, N = pack_infos.shape[0], depth.shape[0]
    m = u.shape[-1]
    uu = u.to(dtype).expand(P, m)
    r['pos'], r['cdf'] = torch.empty(P, m, dtype=torch.int64), torch.empty(N, dtype=dtype)
    r['blidx_fine'] = torch.empty(P, m, dtype=torch.int64)
    r['blidx_merged'] = torch.empty(N + P * m, dtype=torch.int64)
    for p, (b, n) in enumerate(pack_infos.tolist()):
        cdf = pack_cdf(r['alpha'][b:b + n].clone())
        pos = torch.searchsorted(cdf, uu[p].contiguous(), right=False).clamp_max(n - 1)
        r['pos'][p], r['cdf'][b:b + n], r['blidx_fine'][p] = pos, cdf, blidx[b + pos]
    r['blidx_merged'][r['pidx_old']] = blidx
    r['blidx_merged'][r['pidx_fine']] = r['blidx_fine']
    return r


def cdf_tau(r32, r64):
    """4 x the largest |cdf32 - cdf64| of two runs of the restatement on the same inputs"""
    return 4.0 * (r32['cdf'].double() - r64['cdf']).abs().max().item()


def proven_ties(cdf64, pack_infos, u, tau):
    """bool [P, m]: some float64 CDF knot of pack p lies within tau of u[p, j]"""
    P = pack_infos.shape[0]
    uu = u.double().expand(P, u.shape[-1])
    out = torch.zeros(uu.shape, dtype=torch.bool)
    for p, (b, n) in enumerate(pack_infos.tolist()):
        out[p] = ((cdf64[b:b + n][None, :] - uu[p][:, None]).abs() <= tau).any(dim=1)
    return out


def upsample_loop(sdf_fn, rays_o, rays_d, depth, blidx, pack_infos, num_fine, factors, upsample_inv_s, use_estimate, u,
                  dtype=torch.float32, ties=False):
    """the unperturbed up-sampling loop of the forest drivers with sdf = sdf_fn(points [n, 3] in `dtype`): rays_o, rays_d [P, 3] of
    the packs, depth, blidx [N] the marched samples -> dict(fine [P, S m] sorted per pack, blidx [P, S m] in that order, cdfs = the
    CDF of every stage, and with `ties` (a float64 run) taus = one tau per stage and excused bool [P, S m]: the new depth is a proven
    tie of its stage, or it took its label from a sample that is excused -- a label that rounding may decide; excused_union bool [N + P S m] =
    the same for every sample of the union behind the last stage, in its order (False at the samples the loop started from).
    A stage's tau is
    4 x the largest |cdf32 - cdf64| on that stage's own inputs: the float32 stage is run on the float64 loop's samples rounded to
    float32, with the SDF evaluated in float32 there)"""
    o, v = rays_o.cpu().to(dtype), rays_d.cpu().to(dtype)
    d, bl, pi = depth.cpu().to(dtype), blidx.cpu(), pack_infos.cpu()
    taint = torch.zeros_like(bl, dtype=torch.bool)
    m = num_fine // 2 * 2 + 1

    def sdf_at(t, pinfo):
        ridx = torch.repeat_interleave(torch.arange(pinfo.shape[0]), pinfo[:, 1])
        return sdf_fn(o[ridx] + v[ridx] * t[:, None])

    o32, v32 = o.float(), v.float()
    fines, labels, excused, cdfs, taus = [], [], [], [], []
    for i, f in enumerate(factors):
        r = stage(d, sdf_at(d, pi), bl, pi, u, upsample_inv_s * f, use_estimate, dtype)
        first = pi[:, :1]
        ex = taint[first + r['pos']]
        if ties:
            ridx = torch.repeat_interleave(torch.arange(pi.shape[0]), pi[:, 1])
            d32 = d.float()
            r32 = stage(d32, sdf_fn(o32[ridx] + v32[ridx] * d32[:, None]), bl, pi, u, upsample_inv_s * f, use_estimate, torch.float32)
            taus.append(cdf_tau(r32, r))
            ex = ex | proven_ties(r['cdf'], pi, u, taus[-1])
        fines.append(r['fine']), labels.append(r['blidx_fine']), excused.append(ex), cdfs.append(r['cdf'])
        new_taint = torch.empty(r['merged'].shape[0], dtype=torch.bool)
        new_taint[r['pidx_old']], new_taint[r['pidx_fine']] = taint, ex
        d, bl, pi, taint = r['merged'], r['blidx_merged'], r['pack_infos_out'], new_taint
    fine, order = torch.cat(fines, -1).sort(dim=-1, stable=True)
    return dict(fine=fine, blidx=torch.cat(labels, -1).gather(-1, order), excused=torch.cat(excused, -1).gather(-1, order), cdfs=cdfs,
                taus=taus, excused_union=taint)


def labels_every(pack_infos, every=3, base=0):
    """labels that change every `every` samples inside a pack (and differ between neighbouring packs)"""
    out = torch.empty(int(pack_infos[:, 1].sum()), dtype=torch.int64)
    for p, (b, n) in enumerate(pack_infos.tolist()):
        out[b:b + n] = base + 1000 * p + torch.arange(n) // every
    return out


def linear_steps(near, entry, exit, seg_pack_infos, step_size=0.01, step_size_factor=1.0, min_steps=2, max_steps=512):
    """the unperturbed linear stepper, one segment at a time in float32 arithmetic as the library does it: rung k of ray r sits at
    near_r + k step; a segment takes the rungs trunc((entry - near) / step) .. trunc((exit - near) / step), their number clamped to
    [min_steps, max_steps] -> (t, deltas, ridx, ray_pack_infos, sidx, seg_pack_infos_out) as lists / arrays"""
    step = np.float32(step_size * step_size_factor)
    t, ridx, sidx, n_seg, n_ray = [], [], [], [], []
    s = 0
    for r, (b, n) in enumerate(np.asarray(seg_pack_infos).tolist()):
        total = 0
        for k in range(b, b + n):
            nr = np.float32(near[r])
            i0 = int(np.trunc(np.float32(np.float32(entry[k]) - nr) / step))
            i1 = int(np.trunc(np.float32(np.float32(exit[k]) - nr) / step)) + 1
            cnt = min(max(i1 - i0, min_steps), max_steps)
            for i in range(i0, i0 + cnt):
                t.append(np.float32(nr + np.float32(i) * step)), ridx.append(r), sidx.append(s)
            n_seg.append(cnt)
            total += cnt
            s += 1
        n_ray.append(total)
    first = lambda c: np.stack([np.cumsum(c) - np.asarray(c), np.asarray(c)], 1).astype(np.int64)
    return (np.asarray(t, np.float32), np.full(len(t), step, np.float32), np.asarray(ridx), first(n_ray), np.asarray(sidx),
            first(n_seg))
