"""The NeRF++ shell sampler restated in plain torch, in float64 or float32 (tests/test_nerfpp_march_cpu.py holds the float32 form
against a recording of the reference's own sampler, tests/golden/ref_nerfpp_march.npz; tests/test_nerfpp_march_gpu.py judges the HIP
kernels and the project's chain against the float64 form), the ray sets of those tests, and ``near_ties``: the number of (ray, shell)
decisions that float32 and float64 could take differently.  No GPU, no library."""
import math

import numpy as np
import torch

AABB = [[-1.0, -2.0, -0.5], [1.0, 2.0, 0.5]]
MODES = ("box", "ellipsoid", "cube", "spherical")
INTERVALS = ("inverse_proportional", "logarithm", "logarithm_with_inverse_prop_input")
TIE = 1e-4


def shell_table(radius_scale_min, radius_scale_max, max_steps, interval_type, device=None):
    """the table both routes build: (radii float32 [N], step, log_min, log_max) -- N is what arange returns, not max_steps"""
    if interval_type == "inverse_proportional":
        a, b = 1.0 / radius_scale_min, 1.0 / radius_scale_max
        lo = hi = None
    else:
        a, b = lo, hi = np.log10(radius_scale_min), np.log10(radius_scale_max)
    step = (b - a) / max_steps
    return torch.arange(a, b, step, device=device), step, lo, hi


def last_radius(radius_scale_max, include_inf_distance):
    return 1.0e10 if include_inf_distance else radius_scale_max


def _box(o, d, r):
    """o, d [R, 1, 3], r [R, M] -> (t [R, M] with NaN for a miss, t_near, t_far)"""
    a = (-r[..., None] - o) / d
    b = (r[..., None] - o) / d
    t_near = torch.minimum(a, b).max(dim=-1).values
    t_far = torch.maximum(a, b).min(dim=-1).values
    hit = (t_far > t_near) & (t_far > 0)
    return torch.where(hit, t_far, torch.full_like(t_far, math.nan)), t_near, t_far


def _sphere(o, d, r):
    """-> (t [R, M], discriminant, pv^2)"""
    pp, vv, pv = (o * o).sum(-1), (d * d).sum(-1), (o * d).sum(-1)
    disc = pv * pv - vv * (pp - r * r)
    return (disc.sqrt() - pv) / vv, disc, (pv * pv).expand_as(disc)


def _shells(aabb, rays_o, rays_d, radii, noise, step, last, mode, interval, dtype):
    """every ray against every shell: dict(t_ext [R, N + 1], r_reci, r_log [R, N], the normalised ray, the geometry near_ties reads)"""
    aabb, o, d = aabb.to(dtype), rays_o.to(dtype), rays_d.to(dtype)
    R, N = o.shape[0], radii.shape[0]
    c, h, stretch = (aabb[1] + aabb[0]) / 2, (aabb[1] - aabb[0]) / 2, aabb[1] - aabb[0]
    tab = radii.to(dtype)[None, :].expand(R, N)
    r_log = None
    if interval == "inverse_proportional":
        r_reci = tab if noise is None else (tab + noise.to(dtype) * step).clamp(1e-5)
        r = 1 / r_reci
    else:
        r_log = tab if noise is None else tab + noise.to(dtype) * step
        r = 10 ** r_log
        r_reci = 1 / r
    r_ext = torch.cat([r, torch.full((R, 1), last, dtype=dtype, device=o.device)], -1)
    o_n, d_n = (o - c) / h, d / h
    if mode in ("box", "ellipsoid"):
        io, idir, rr = o_n[:, None], d_n[:, None], r_ext
    else:
        io, idir, rr = o[:, None], d[:, None], r_ext * stretch.min()
    out = dict(r_reci=r_reci, r_log=r_log, o=o, d=d, o_n=o_n, d_n=d_n, c=c, h=h)
    if mode in ("box", "cube"):
        out["t_ext"], out["t_near"], out["t_far"] = _box(io, idir, rr)
    else:
        out["t_ext"], out["disc"], out["pv2"] = _sphere(io, idir, rr)
    return out


def march(aabb, rays_o, rays_d, t_min, radii, noise, step, last, mode, interval, log_min, log_max, dtype=torch.float64):
    """the sampler in ``dtype``: dict(ridx_hit, samples [S, 4], depth_samples, deltas, ridx, pack_infos, pidx = the shell of every
    sample), or None without a valid sample.
    ``radii`` float32 [N] and ``noise`` float32 [R, N] | None are the values both routes start from."""
    g = _shells(aabb, rays_o, rays_d, radii, noise, step, last, mode, interval, dtype)
    t_ext = g["t_ext"]
    t, deltas = t_ext[:, :-1], t_ext[:, 1:] - t_ext[:, :-1]
    if mode in ("box", "ellipsoid"):
        p = g["o_n"][:, None] + g["d_n"][:, None] * t[..., None]
        x_dir, reci, lg = p * g["r_reci"][..., None], g["r_reci"], g["r_log"]
    else:
        p = ((g["o"][:, None] + g["d"][:, None] * t[..., None]) - g["c"]) / g["h"]
        n = p.norm(dim=-1)
        x_dir, reci, lg = p / n.clamp_min(1e-12)[..., None], 1 / n, torch.log10(n)
    if interval == "logarithm":
        w = (lg - log_min) / (log_max - log_min) * 2 - 1
    else:
        w = reci * 2 - 1
    x = torch.cat([x_dir, w[..., None]], -1)
    valid = ~(torch.isnan(t) | (t < t_min.to(dtype)[:, None]))
    ridx, pidx = valid.nonzero().t()
    if ridx.numel() == 0:
        return None
    n_per_ray = valid.sum(-1)
    ridx_hit = n_per_ray.nonzero()[:, 0]
    pack_infos = torch.stack([n_per_ray.cumsum(0) - n_per_ray, n_per_ray], 1)[ridx_hit]
    return dict(ridx_hit=ridx_hit, samples=x[ridx, pidx], depth_samples=t[ridx, pidx], deltas=deltas[ridx, pidx], ridx=ridx,
                pack_infos=pack_infos, pidx=pidx)


def near_ties(aabb, rays_o, rays_d, t_min, radii, noise, step, last, mode, interval):
    """in float64: the (ray, shell) pairs, the closing shell included, whose validity float32 could decide the other way --
    |t - t_min| <= 1e-4 max(1, |t|); a box with |t_far - t_near| <= 1e-4 or |t_far| <= 1e-4; a sphere whose discriminant is within
    1e-4 pv^2 of zero"""
    g = _shells(aabb, rays_o, rays_d, radii, noise, step, last, mode, interval, torch.float64)
    t = g["t_ext"][:, :-1]
    tm = t_min.double()[:, None]
    tie = (t - tm).abs() <= TIE * t.abs().clamp_min(1.0)
    n = int(tie.sum())
    if "t_far" in g:
        n += int(((g["t_far"] - g["t_near"]).abs() <= TIE).sum()) + int((g["t_far"].abs() <= TIE).sum())
    else:
        n += int((g["disc"].abs() <= TIE * g["pv2"]).sum())
    return n


# ---- ray sets --------------------------------------------------------------------------------------------------------------------
def golden_rays():
    """the 12 rays of the recording: origins inside the box, about 6x and about 30x outside it; non-unit directions; one ray with one
    zero direction component and one with two; t_min of 0, small, mid-range and beyond the last shell"""
    o = torch.tensor([[0.1, -0.3, 0.05], [-0.5, 1.2, -0.2], [0.7, 0.4, 0.3], [0.0, 0.0, 0.0],
                      [5.5, -3.0, 1.0], [-2.0, 11.0, 0.7], [1.5, 4.0, -3.2], [-6.1, -2.5, 0.4],
                      [28.0, 10.0, -4.0], [-9.0, -55.0, 2.0], [3.0, 7.0, 14.5], [0.3, 0.2, -0.1]], dtype=torch.float32)
    d = torch.tensor([[0.9, 0.3, -0.2], [-1.7, 0.4, 0.6], [0.2, -2.5, 0.1], [0.3, 0.4, 1.3],
                      [-1.0, 0.6, -0.1], [0.5, -1.9, 0.05], [-0.4, -0.8, 0.7], [1.2, 0.5, 0.0],
                      [-2.0, -0.7, 0.3], [0.3, 1.6, -0.1], [-0.2, -0.5, -1.1], [0.0, 1.4, 0.0]], dtype=torch.float32)
    t_min = torch.tensor([0.0, 0.05, 9.0, 1e6, 2.0, 0.0, 30.0, 1e6, 0.5, 200.0, 1e6, 0.0], dtype=torch.float32)
    return torch.tensor(AABB, dtype=torch.float32), o, d, t_min


def rays(R, seed, kind="mixed"):
    """the GPU tests' rays through the box AABB, float32 on the CPU: (aabb, rays_o, rays_d, t_min).
    'mixed': a third of the origins inside the box, a third about 6x and a third about 30x outside, non-unit directions, every 7th ray
    with one zero direction component and every 11th with two; t_min cycling through 0, small, mid-range and beyond the last shell.
    'inside': every origin inside the innermost shell of every mode, t_min 0 -- every shell valid.  'empty_edges': 'mixed' with the first two, a middle pair and the
    last two rays cut off by t_min.  'none': every ray cut off."""
    g = torch.Generator().manual_seed(seed)
    aabb = torch.tensor(AABB, dtype=torch.float32)
    c, h = (aabb[1] + aabb[0]) / 2, (aabb[1] - aabb[0]) / 2
    u = torch.rand(R, 3, generator=g) * 2 - 1
    d = torch.randn(R, 3, generator=g) * (0.5 + 2.0 * torch.rand(R, 1, generator=g))
    idx = torch.arange(R)
    if kind == "inside":
        o = c + 0.4 * u * h                                    # inside the first shell of every mode, the unit sphere of 'spherical' included
        t_min = torch.zeros(R)
    else:
        scale = torch.tensor([0.9, 6.0, 30.0])[idx % 3][:, None]
        o = c + scale * u * h
        d[idx % 7 == 3, 2] = 0.0
        two = idx % 11 == 5
        d[two, 0] = 0.0
        d[two, 2] = 0.0
        t_min = torch.tensor([0.0, 0.07, 11.0, 1e7])[(idx // 3 + idx) % 4] * (0.5 + torch.rand(R, generator=g))
        if kind == "empty_edges":
            cut = torch.tensor([0, 1, R // 2, R // 2 + 1, R - 2, R - 1]).clamp(0, R - 1)
            t_min[cut] = 1e12
        elif kind == "none":
            t_min[:] = 1e12
    return aabb, o.float().contiguous(), d.float().contiguous(), t_min.float().contiguous()


def face_plane_case():
    """an axis-parallel ray that starts exactly ON a face plane of one shell: radius_scale_min=1, radius_scale_max=4, max_steps=6,
    'inverse_proportional' gives the table 1, .875, .75, .625, .5, .375 (all exact), so shell 4 has r = 2 whatever the division rounds
    like; the box is centred with half-extent 1 in x and its shortest side is 1, so 'box' and 'cube' both put that shell's face at x = 2.
    The ray starts there and runs along +y: the x slab of shell 4 is 0 / 0 = NaN, the shells inside it are missed (-inf), the one
    outside is hit.  A second, ordinary ray keeps the case from being a single pack.  -> (aabb, rays_o, rays_d, t_min, march keywords)"""
    aabb = torch.tensor(AABB, dtype=torch.float32)
    o = torch.tensor([[2.0, 0.3, 0.1], [0.2, -0.4, 0.1]], dtype=torch.float32)
    d = torch.tensor([[0.0, 1.4, 0.0], [0.6, 0.8, -0.3]], dtype=torch.float32)
    return aabb, o, d, torch.zeros(2), dict(radius_scale_min=1.0, radius_scale_max=4.0, max_steps=6, interval_type="inverse_proportional")
