"""Restatement of one packed up-sampling stage of the NeuS occupancy-march queries and of their up-sampling loop, written pack by
pack from the stage's description in include/nr3d_hip.h (interval opacity -> early-stopped weights -> exclusive sum, divided
afterwards -> inversion with the pmf rule and one fma -> union with a new depth before an equal old one), with a dtype argument:
the float32 run is pinned to the CPU oracle's pack ops by tests/test_neus_packed_cpu.py, the float64 run on the same float32
inputs is what the HIP kernel's error is measured against, and the distance between the two runs is the yardstick for that error.

Also the packs on the analytic sphere of tests/neus_coarse_ref.py that the packed tests share."""
import numpy as np
import torch

import neus_coarse_ref as cref

EARLY_STOP, PMF_MIN, MASS_MIN = 1e-4, 1e-5, 1e-5
SLOPE_CLAMP, SLOPE_EPS, ALPHA_EPS = -10.0, 1e-5, 1e-5
# a wrong kernel, for tests/test_upsample_decisions_cpu.py alone: the early stop is honoured in the first chunk of 64 elements only
STOP_FIRST_CHUNK_ONLY = False
# torch's CPU cumsum / cumprod keep a float32 row's running value in double.  True: the product and the sum run in order IN the dtype,
# as the oracle's pack ops do.  Next to cdf = 1 the difference is an ulp of the CDF, which an inverted bin with a pmf of 1e-4 turns
# into 1e-3 of the bin: tests/upsample_decision_inputs.py, which inverts such bins, sets it; the parity inputs do not notice.
SUMS_IN_DTYPE = False


def _fma(a, b, c):
    """a b + c with one rounding: in float64 the product of two float32 values is exact"""
    if a.dtype == torch.float32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def _cumsum(x):
    return torch.from_numpy(np.cumsum(x.numpy(), dtype=x.numpy().dtype)) if SUMS_IN_DTYPE else torch.cumsum(x, 0)


def _cumprod(x):
    return torch.from_numpy(np.cumprod(x.numpy(), dtype=x.numpy().dtype)) if SUMS_IN_DTYPE else torch.cumprod(x, 0)


def alpha_of(d, s, inv_s, use_estimate):
    """the opacity of every element of ONE pack (d, s [n] in the dtype to compute in); the last element closes no interval: 0"""
    n = d.shape[0]
    alpha = torch.zeros_like(s)
    if n < 2:
        return alpha
    if not use_estimate:
        c = torch.sigmoid(s * inv_s)
        c_prev, c_next = c[:-1], c[1:]
    else:
        d_sdf, delta = s[1:] - s[:-1], d[1:] - d[:-1]
        slope = d_sdf / (delta + SLOPE_EPS)
        before = torch.cat([torch.zeros_like(slope[:1]), slope[:-1]])
        sl = torch.minimum(before, slope).clamp(SLOPE_CLAMP, 0.0)
        mid, half = s[:-1] + d_sdf * 0.5, sl * delta * 0.5
        c_prev, c_next = torch.sigmoid((mid - half) * inv_s), torch.sigmoid((mid + half) * inv_s)
    alpha[:-1] = ((c_prev - c_next) / (c_prev + ALPHA_EPS)).clamp_min(0)
    return alpha


def pack_stage(d, alpha, u):
    """ONE pack from its opacities on: d, alpha [n], u [m] in one dtype -> dict(fine [m], lb [m] = the number of old depths below
    every new one, wsum, t_margin = the smallest |T / 1e-4 - 1| over the transmittances up to the early stop, pmf [m] = the pmf of
    every inverted bin (inf where none is read))"""
    n = d.shape[0]
    keep = torch.where(alpha <= 0, torch.ones_like(alpha), 1.0 - alpha)
    T = torch.cat([torch.ones_like(keep[:1]), _cumprod(keep)[:-1]])
    below = (T < EARLY_STOP).nonzero()
    stop = int(below[0]) if below.numel() else n
    if STOP_FIRST_CHUNK_ONLY and stop >= 64:
        stop = n
    w = alpha * T
    w[stop:] = 0
    cdf = torch.cat([torch.zeros_like(w[:1]), _cumsum(w)[:-1]])
    cdf = cdf / cdf[-1].clamp_min(MASS_MIN)
    pos = torch.searchsorted(cdf, u.contiguous(), right=False).clamp_max(n - 1)
    lo = (pos - 1).clamp_min(0)
    c0, pmf, d0 = cdf[lo], cdf[pos] - cdf[lo], d[lo]
    lerp = _fma((u - c0) / torch.where(pmf < PMF_MIN, torch.ones_like(pmf), pmf), d[pos] - d0, d0)
    fine = torch.where(pos == 0, d[0].expand_as(u), torch.where(pmf < PMF_MIN, d0, lerp))
    fine = torch.cummax(fine, 0).values
    return dict(fine=fine, lb=torch.searchsorted(d.contiguous(), fine.contiguous(), right=False), wsum=w.sum(),
                t_margin=(T[:min(stop + 1, n)] / EARLY_STOP - 1).abs().min(),
                pmf=torch.where(pos == 0, torch.full_like(pmf, float('inf')), pmf))


def merge_positions(first, n, lb, p):
    """where pack p's n old and m new elements go in the merged buffer: -> (start, index of every old, of every new element)"""
    m = lb.shape[0]
    start = first + p * m
    new = start + lb + torch.arange(m)
    old = start + torch.arange(n) + torch.searchsorted(lb.contiguous(), torch.arange(n), right=True)
    return start, old, new


def stage(depth, sdf, pack_infos, u, inv_s, use_estimate, dtype=torch.float32, alpha=None):
    """depth, sdf [N] packed, pack_infos int64 [P, 2] tiling [0, N), u [m] or [P, m] (taken as they are, converted to `dtype`;
    `alpha` [N], when given, replaces the opacities) -> dict(fine [P, m], merged, sdf_merged [N + P m] (NaN at the new depths'
    places), pidx_old [N], pidx_fine [P, m], pack_infos_out [P, 2], wsum, t_margin [P], pmf [P, m], alpha [N])"""
    d_all, s_all, u = depth.to(dtype), sdf.to(dtype), u.to(dtype)
    P, N = pack_infos.shape[0], depth.shape[0]
    m = u.shape[-1]
    u = u.expand(P, m)
    out = dict(fine=torch.empty(P, m, dtype=dtype), merged=torch.empty(N + P * m, dtype=dtype),
               sdf_merged=torch.full((N + P * m,), float('nan'), dtype=dtype), pidx_old=torch.empty(N, dtype=torch.int64),
               pidx_fine=torch.empty(P, m, dtype=torch.int64), pack_infos_out=torch.empty(P, 2, dtype=torch.int64),
               wsum=torch.empty(P, dtype=dtype), t_margin=torch.empty(P, dtype=dtype), pmf=torch.empty(P, m, dtype=dtype),
               alpha=torch.empty(N, dtype=dtype))
    for p, (b, n) in enumerate(pack_infos.tolist()):
        d, s = d_all[b:b + n], s_all[b:b + n]
        a = alpha_of(d, s, inv_s, use_estimate) if alpha is None else alpha[b:b + n].to(dtype)
        r = pack_stage(d, a, u[p])
        start, old, new = merge_positions(b, n, r['lb'], p)
        out['fine'][p], out['wsum'][p], out['t_margin'][p], out['pmf'][p], out['alpha'][b:b + n] = r['fine'], r['wsum'], r['t_margin'], r['pmf'], a
        out['merged'][old], out['merged'][new], out['sdf_merged'][old] = d, r['fine'], s
        out['pidx_old'][b:b + n], out['pidx_fine'][p] = old, new
        out['pack_infos_out'][p, 0], out['pack_infos_out'][p, 1] = start, n + m
    return out


def upsample_loop(rays_o, rays_d, depth, pack_infos, num_fine, factors, upsample_inv_s, use_estimate, dtype=torch.float32,
                  radius=cref.RADIUS):
    """the unperturbed loop of the march-occ drivers' up-sampling on the analytic sphere sdf = |o + t d| - radius, every step in
    `dtype`: rays_o, rays_d [P, 3] of the packs, depth [N] the marched depths -> the fine depths [P, len(factors) m] sorted per pack,
    m = num_fine // 2 * 2 + 1"""
    o, v = rays_o.cpu().to(dtype), rays_d.cpu().to(dtype)
    d, pi = depth.cpu().to(dtype), pack_infos.cpu()
    m = num_fine // 2 * 2 + 1
    u = cref.shared_u(m, dtype)

    def sdf_at(t, pinfo):
        ridx = torch.repeat_interleave(torch.arange(pinfo.shape[0]), pinfo[:, 1])
        return (o[ridx] + v[ridx] * t[:, None]).norm(dim=-1) - radius

    fines = []
    for i, f in enumerate(factors):
        r = stage(d, sdf_at(d, pi), pi, u, upsample_inv_s * f, use_estimate, dtype)
        fines.append(r['fine'])
        d, pi = r['merged'], r['pack_infos_out']
    return torch.cat(fines, -1).sort(dim=-1).values


def sphere_packs(lengths, near=cref.NEAR, far=cref.FAR):
    """one pack per entry of `lengths`: uniform depths in [near, far] (a pack of one element: near) on the rays of fan_rays(4), in
    turn, and the sphere's sdf there -> (depth [N], sdf [N], pack_infos int64 [P, 2]), float32"""
    rays = cref.fan_rays(4)
    depth, sdf, first = [], [], 0
    pack_infos = torch.empty(len(lengths), 2, dtype=torch.int64)
    for p, n in enumerate(lengths):
        o, v = rays['rays_o'][p % 16], rays['rays_d'][p % 16]
        t = torch.linspace(near, far, n) if n > 1 else torch.full((1,), near)
        depth.append(t)
        sdf.append((o[None, :] + v[None, :] * t[:, None]).norm(dim=-1) - cref.RADIUS)
        pack_infos[p, 0], pack_infos[p, 1] = first, n
        first += n
    return torch.cat(depth).contiguous(), torch.cat(sdf).contiguous(), pack_infos


def parity_lengths(lds_row, m):
    """the pack lengths of the GPU parity cases, in a fixed shuffled order (LDS and global packs share workgroups)"""
    lengths = [1, 2, 3, 5, 17, 33, 63, 64, 65, 128, 129, 200, lds_row - m, lds_row - m + 1, 2 * lds_row + 7]
    order = torch.randperm(len(lengths), generator=torch.Generator().manual_seed(11)).tolist()
    return [lengths[i] for i in order]


def exact_packs(r64, pack_infos):
    """packs whose `fine` no rounding can move: one element, or so little mass (float64 sum below 1e-7 against the 1e-5 that the
    CDF is divided by at least) that every pmf is far below 1e-5"""
    return (pack_infos[:, 1] == 1) | (r64['wsum'] < 1e-7)


def check_preconditions(r64, pack_infos):
    """what the parity comparison of `fine` needs, on the float64 run: mass where an inverse CDF is compared by tolerance, no early
    stop and no pmf rule that rounding could decide"""
    long_packs = pack_infos[:, 1] >= 17
    assert r64['wsum'][long_packs].min().item() >= 0.99, f"weight sum {r64['wsum'][long_packs].min().item()}"
    assert r64['t_margin'].min().item() > 1e-3, f"a transmittance within {r64['t_margin'].min().item():.2e} of the early stop"
    pmf = r64['pmf'][~exact_packs(r64, pack_infos)]
    assert not ((pmf >= 0.5e-5) & (pmf <= 2e-5)).any(), "an inverted bin's pmf next to 1e-5"


PARITY_M, PARITY_INV_S = (1, 9, 65), (64, 256, 1024)
