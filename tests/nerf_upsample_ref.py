"""Restatement of the two packed stages of the NeRF march + up-sample ray query, written loop-free from their description in
include/nr3d_hip.h -- (a) ``merge``: the union of every ray's coarse row with its marched pack, its differences, ray indices and
positions; (b) ``stage``: opacity -> inclusive sum, divided afterwards -> inversion with the pmf rule and one fma -> running maximum
-> union with the coarse row, or the interval ends without one -- with a dtype argument: the float32 run is pinned to the CPU
oracle's pack ops by tests/test_nerf_upsample_cpu.py, the float64 run on the same float32 inputs is what the HIP kernel's error is
measured against, and the distance between the two runs is the yardstick for that error.

The float32 run evaluates the opacity as the op chain does, 1 - exp(-sigma delta); the kernel's -expm1(-sigma delta) is the same
quantity without that expression's cancellation, and the float64 run is the common truth of both.

Packs are handled as padded rows [P, longest pack]; nothing loops over packs or elements.  The one sum runs through numpy: its
``cumsum`` adds strictly in order IN the array's dtype, which is what the oracle's ``packed_cumsum`` does, whereas torch's CPU cumsum
keeps a float32 row's running sum in double.

Also the inputs the tests share: packs of uniform depths through a soft density shell on the rays of neus_coarse_ref.fan_rays(4)."""
import numpy as np
import torch

import neus_coarse_ref as cref

PMF_MIN, MASS_MIN = 1e-5, 1e-5
# The shell: sigma = SIGMA (1 + SKEW z) exp(-((|x| - RADIUS) / WIDTH)^2).  A ray crosses a spherical shell twice, in mirror image: with
# equal mass in both crossings the CDF rests at 1/2 between them, which is a CDF position of every odd m, and a peak of 60 saturates
# the opacity of the short packs (sigma delta >> 1), which puts the CDF's plateaus on small fractions -- other CDF positions.  Hence
# the skew along z and the low peak: the plateau sits near 0.36, between 23/66 and 24/66, and no opacity comes near 1.
# tests/test_nerf_upsample_cpu.py asserts the preconditions of the parity cases on these numbers and prints the margins.
SHELL_RADIUS, SHELL_WIDTH, SHELL_SIGMA, SHELL_SKEW = 0.62, 0.08, 3.0, 0.48


def _fma(a, b, c):
    """a b + c with one rounding: in float64 the product of two float32 values is exact"""
    if a.dtype == torch.float32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def _cumsum(x):
    """along the last dim, added in order in x's own dtype"""
    return torch.from_numpy(np.cumsum(x.numpy(), axis=-1, dtype=x.numpy().dtype))


def padded(pack_infos, numel):
    """-> (idx int64 [P, nmax]: the element of every slot of every pack, clamped into [0, numel); mask [P, nmax]: the slot exists)"""
    first, lens = pack_infos[:, 0], pack_infos[:, 1]
    k = torch.arange(int(lens.max()) if lens.numel() else 0)
    mask = k[None, :] < lens[:, None]
    return (first[:, None] + k[None, :]).clamp(0, max(numel - 1, 0)), mask


def packed_diff(x, pack_infos):
    """x[i + 1] - x[i] inside every pack, 0 for its last element (the packs tile x)"""
    d = torch.zeros_like(x)
    d[:-1] = x[1:] - x[:-1]
    last = pack_infos[:, 0] + pack_infos[:, 1] - 1
    d[last[pack_infos[:, 1] > 0]] = 0
    return d


def union_positions(a, b, b_mask=None):
    """rows a [R, na], b [R, nb] (sorted; slots of b outside b_mask do not exist) -> the place inside the row's union of every element
    of a and of b, an element of b BEFORE an equal one of a (the lower bound of b among a) and equal elements of one list in their order"""
    inf = torch.full_like(b, float('inf'))
    b_real = b if b_mask is None else torch.where(b_mask, b, inf)
    pos_a = torch.arange(a.shape[1]) + torch.searchsorted(b_real.contiguous(), a.contiguous(), right=True)
    pos_b = torch.arange(b.shape[1]) + torch.searchsorted(a.contiguous(), b_real.contiguous(), right=False)
    return pos_a, pos_b


def merge(coarse, depth, pack_infos_all, rays_o, rays_d, dtype=torch.float32):
    """(a): coarse [R, nc], depth [N], pack_infos_all int64 [R, 2] (length 0 for a missed ray, tiling [0, N) in ray order),
    rays_o, rays_d [R, 3] -> dict(depths_all, deltas_all, ridx_all, samples_all, pack_infos_out, pidx_coarse [R, nc], pidx_marched [N])"""
    a, t, o, v = coarse.to(dtype), depth.to(dtype), rays_o.to(dtype), rays_d.to(dtype)
    R, nc = a.shape
    N = t.shape[0]
    first, lens = pack_infos_all[:, 0], pack_infos_all[:, 1]
    idx, mask = padded(pack_infos_all, N)
    b = t[idx] if N else t.new_zeros(R, 0)
    pos_a, pos_b = union_positions(a, b, mask)
    begin = torch.arange(R) * nc + first
    pidx_a, pidx_b = begin[:, None] + pos_a, (begin[:, None] + pos_b)[mask]
    depths_all = t.new_empty(R * nc + N)
    depths_all[pidx_a.flatten()], depths_all[pidx_b] = a.flatten(), b[mask]
    pinfo = torch.stack([begin, nc + lens], -1)
    ridx = torch.repeat_interleave(torch.arange(R), pinfo[:, 1])
    return dict(depths_all=depths_all, deltas_all=packed_diff(depths_all, pinfo), ridx_all=ridx,
                samples_all=_fma(v[ridx], depths_all[:, None].expand(-1, 3), o[ridx]), pack_infos_out=pinfo, pidx_coarse=pidx_a,
                pidx_marched=pidx_b)


def stage(depth, sigma, delta, pack_infos, u, coarse=None, coarse_row=None, dtype=torch.float32, alpha=None):
    """(b): depth, sigma, delta [N] packed, pack_infos int64 [P, 2] tiling [0, N), u [m] or [P, m], coarse [Rc, nc] with coarse_row [P]
    (None: row p) -> dict(fine [P, m]; merged, deltas [P, nc + m] or [P, m - 1]; cdf [P, nmax] (inf past the pack), mass [P] = c_{n-1},
    pos [P, m] = the bin of every u, pmf [P, m] = its pmf (inf where none is read), u_gap [P, m] = the distance from u to the nearest
    CDF value of its pack, alpha [N], and with coarse pos_coarse [P, nc], pos_fine [P, m] = the places in the union)"""
    d_all, u = depth.to(dtype), u.to(dtype)
    P, N = pack_infos.shape[0], depth.shape[0]
    m = u.shape[-1]
    u = u.expand(P, m).contiguous()
    a_all = (1 - torch.exp(-(sigma.to(dtype) * delta.to(dtype)))) if alpha is None else alpha.to(dtype)
    idx, mask = padded(pack_infos, N)
    lens = pack_infos[:, 1]
    d = d_all[idx]
    c = _cumsum(torch.where(mask, a_all[idx], torch.zeros_like(d)))
    mass = c.gather(-1, (lens - 1).clamp_min(0)[:, None])
    cdf = torch.where(mask, c / mass.clamp_min(MASS_MIN), torch.full_like(c, float('inf')))
    pos = torch.minimum(torch.searchsorted(cdf.contiguous(), u, right=False), (lens - 1)[:, None])
    lo = (pos - 1).clamp_min(0)
    c0, d0 = cdf.gather(-1, lo), d.gather(-1, lo)
    pmf = cdf.gather(-1, pos) - c0
    small = pmf < PMF_MIN
    lerp = _fma((u - c0) / torch.where(small, torch.ones_like(pmf), pmf), d.gather(-1, pos) - d0, d0)
    fine = torch.where(pos == 0, d[:, :1].expand_as(u), torch.where(small, d0, lerp))
    fine = torch.cummax(fine, -1).values
    gap = (cdf[:, None, :] - u[:, :, None]).abs().amin(-1)
    out = dict(fine=fine, cdf=cdf, mass=mass[:, 0], pos=pos, pmf=torch.where(pos == 0, torch.full_like(pmf, float('inf')), pmf),
               u_gap=gap, alpha=a_all)
    if coarse is None:
        df = fine[:, 1:] - fine[:, :-1]
        out.update(merged=fine[:, :-1] + df, deltas=df)
        return out
    k = coarse.to(dtype)[torch.arange(P) if coarse_row is None else coarse_row]
    pos_k, pos_f = union_positions(k, fine)
    merged = torch.empty(P, k.shape[1] + m, dtype=dtype)
    merged.scatter_(-1, pos_k, k)
    merged.scatter_(-1, pos_f, fine)
    out.update(merged=merged, deltas=torch.cat([merged[:, 1:] - merged[:, :-1], torch.zeros_like(merged[:, :1])], -1), pos_coarse=pos_k,
               pos_fine=pos_f)
    return out


def shell_sigma(x, dtype=torch.float32):
    """the density of the soft shell at points x [..., 3]"""
    x = x.to(dtype)
    return SHELL_SIGMA * (1 + SHELL_SKEW * x[..., 2]) * torch.exp(-((x.norm(dim=-1) - SHELL_RADIUS) / SHELL_WIDTH) ** 2)


def soft_shell_packs(lengths, near=cref.NEAR, far=cref.FAR):
    """one pack per entry of `lengths`: uniform depths in [near, far] (a pack of one element: near) on the rays of fan_rays(4), in
    turn, the shell's density there and packed_diff of the depths
    -> (depth [N], sigma [N], delta [N], pack_infos int64 [P, 2], rays_o [P, 3], rays_d [P, 3]), float32"""
    rays = cref.fan_rays(4)
    lens = torch.tensor(lengths, dtype=torch.int64)
    P = lens.numel()
    pack_infos = torch.stack([torch.cumsum(lens, 0) - lens, lens], -1)
    o, v = rays['rays_o'][torch.arange(P) % 16], rays['rays_d'][torch.arange(P) % 16]
    which = torch.repeat_interleave(torch.arange(P), lens)
    k = (torch.arange(int(lens.sum())) - pack_infos[which, 0]).float()
    steps = (lens - 1).clamp_min(1).float()[which]
    depth = (near + (far - near) * (k / steps)).float().contiguous()
    sigma = shell_sigma(o[which] + v[which] * depth[:, None]).contiguous()
    return depth, sigma, packed_diff(depth, pack_infos), pack_infos, o.contiguous(), v.contiguous()


def coarse_rows(near, far, num_coarse):
    """near, far [R] -> [R, num_coarse]: the mid-points of num_coarse linear steps from near to far (what the driver puts on every ray)"""
    dt = ((far - near) / num_coarse)[:, None]
    return (torch.addcmul(near[:, None], torch.arange(num_coarse, device=near.device).to(near.dtype)[None, :], dt) + dt / 2.).contiguous()


def shared_u(m, dtype=torch.float32):
    return torch.linspace(0., 1., m + 2, dtype=dtype)[1:-1].contiguous()


def per_pack_u(P, m, seed=3):
    """one stratified (hence sorted) row of positions per pack, seeded"""
    r = torch.rand(P, m, generator=torch.Generator().manual_seed(seed))
    return ((torch.arange(m)[None, :] + 0.1 + 0.8 * r) / m).float().contiguous()


def parity_lengths(lds_row, m, nc):
    """the pack lengths of the GPU parity cases, in a fixed shuffled order (LDS and global packs share workgroups)"""
    edge = lds_row - m - nc
    lengths = [1, 2, 3, 5, 17, 33, 63, 64, 65, 128, 129, 200, edge, edge + 1, 2 * lds_row + 7]
    order = torch.randperm(len(lengths), generator=torch.Generator().manual_seed(11)).tolist()
    return [lengths[i] for i in order]


def check_preconditions(r64, pack_infos):
    """what the parity comparison of `fine` needs, on the float64 run: mass where an inverse CDF is compared by tolerance, and no bin
    search or pmf rule that rounding could decide.  -> the three margins"""
    long_packs = pack_infos[:, 1] >= 17
    mass = r64['mass'][long_packs].min().item() if long_packs.any() else float('inf')
    assert mass >= 0.05, f"a pack of 17 elements or more with c_(n-1) = {mass}"
    pmf = r64['pmf']
    assert not ((pmf >= 0.5e-5) & (pmf <= 2e-5)).any(), "an inverted bin's pmf next to 1e-5"
    gap = r64['u_gap'].min().item()
    assert gap > 1e-6, f"a CDF position within {gap:.2e} of a CDF value"
    near = pmf[torch.isfinite(pmf)]
    return dict(min_mass=mass, min_u_gap=gap, pmf_nearest=(near / 1e-5).log().abs().min().item() if near.numel() else float('inf'))


PARITY_M, PARITY_NC = (1, 9, 65), (0, 16)
