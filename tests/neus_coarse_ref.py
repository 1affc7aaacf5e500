"""Restatement of one up-sampling stage of the vanilla NeuS coarse ray query and of the whole coarse loop, written from the stage's
description in include/nr3d_hip.h (interval opacity -> weights -> CDF -> inversion -> sorted union), with a dtype argument: the
float32 run is pinned to the reference's own results by tests/test_neus_coarse_cpu.py, the float64 run on the same float32 inputs
is what the HIP kernel's error is measured against, and the distance between the two runs is the yardstick for that error.

Also the analytic model and the ray fan the coarse-query tests share."""
import numpy as np
import torch

RADIUS, FORWARD_INV_S = 0.62, 48.0
ORIGIN, NEAR, FAR = (0.0, 0.0, -2.5), 1.5, 3.5


class SphereModel(torch.nn.Module):
    """sdf = |x| - RADIUS with the model protocol of the NeuS ray queries (forward, forward_sdf, forward_inv_s)"""

    def __init__(self, radius=RADIUS, inv_s=FORWARD_INV_S):
        super().__init__()
        self.radius, self.inv_s = radius, inv_s

    def forward_inv_s(self):
        return self.inv_s

    def forward_sdf(self, x, **kw):
        return dict(sdf=x.norm(dim=-1) - self.radius)

    def forward(self, x, nablas_has_grad=False, with_rgb=True, with_normal=True, **kw):
        out = self.forward_sdf(x)
        normal = torch.nn.functional.normalize(x, dim=-1)
        if with_normal:
            out['nablas'] = normal
        if with_rgb:
            out['rgb'] = 0.5 + 0.5 * normal
        return out


def fan_rays(k=8, spread=0.12, device='cpu'):
    """k x k rays from ORIGIN with directions normalize((spread i, spread j, 1)), i, j in [-1, 1] -> ray_tested dict (float32)"""
    g = torch.linspace(-1.0, 1.0, k)
    ii, jj = torch.meshgrid(g, g, indexing='ij')
    d = torch.stack([spread * ii.flatten(), spread * jj.flatten(), torch.ones(k * k)], -1)
    d = (d / d.norm(dim=-1, keepdim=True)).float()
    n = k * k
    return dict(num_rays=n, rays_o=torch.tensor(ORIGIN).expand(n, 3).contiguous().to(device), rays_d=d.to(device),
                near=torch.full((n,), NEAR).to(device), far=torch.full((n,), FAR).to(device),
                rays_inds=torch.arange(n, device=device))


def shared_u(m, dtype=torch.float32):
    return torch.linspace(0., 1., m + 2, dtype=dtype)[1:-1]


def _cumsum(x, dim):
    return torch.from_numpy(np.cumsum(x.numpy(), axis=dim, dtype=x.numpy().dtype))


def _cumprod(x, dim):
    return torch.from_numpy(np.cumprod(x.numpy(), axis=dim, dtype=x.numpy().dtype))


def stage(depth, sdf, u, inv_s, use_estimate, dtype=torch.float32, *, slope_clamp=-10.0, slope_eps=1e-5, alpha_eps=1e-5,
          mass_min=1e-5, den_min=1e-5, sums_in_dtype=False):
    """depth, sdf [R, n], u [m] or [R, m] (all taken as they are and converted to `dtype`) ->
    dict(fine [R, m], wsum [R] = the sum of the weights, cdf [R, n])
    The keyword arguments are the stage's literals (the kernel's values by default): tests/test_upsample_decisions_cpu.py moves them.
    sums_in_dtype: the product and the sums run in order IN `dtype` (torch's CPU cumsum / cumprod / sum keep a float32 row's running
    value in double; next to cdf = 1 the difference is an ulp of the CDF, which an inverted bin with a pmf of 1e-4 turns into 1e-3
    of the bin -- tests/upsample_decision_inputs.py inverts such bins and sets it)"""
    d, s, u = depth.to(dtype), sdf.to(dtype), u.to(dtype)
    u = u.expand(d.shape[0], u.shape[-1]).contiguous()
    n = d.shape[-1]
    if not use_estimate:
        c = torch.sigmoid(s * inv_s)
        c_prev, c_next = c[:, :-1], c[:, 1:]
    else:
        delta = d[:, 1:] - d[:, :-1]
        mid = (s[:, :-1] + s[:, 1:]) * 0.5
        slope = (s[:, 1:] - s[:, :-1]) / (delta + slope_eps)
        before = torch.cat([torch.zeros_like(slope[:, :1]), slope[:, :-1]], -1)
        slope = torch.minimum(before, slope).clamp(slope_clamp, 0.0)
        c_prev = torch.sigmoid((mid + slope * (delta * -0.5)) * inv_s)
        c_next = torch.sigmoid((mid + slope * (delta * 0.5)) * inv_s)
    alpha = ((c_prev - c_next) / (c_prev + alpha_eps)).clamp_min(0)
    keep = torch.cat([torch.ones_like(alpha[:, :1]), (1 + 1e-10) - alpha[:, :-1]], -1)
    cumprod, cumsum = (_cumprod, _cumsum) if sums_in_dtype else (torch.cumprod, torch.cumsum)
    w = alpha * cumprod(keep, -1)
    wsum = cumsum(w, -1)[:, -1:] if sums_in_dtype else w.sum(-1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(w[:, :1]), cumsum(w / wsum.clamp_min(mass_min), -1)], -1)
    k = torch.searchsorted(cdf, u, right=False)
    lo, hi = (k - 1).clamp_min(0), k.clamp_max(n - 1)
    c_lo, c_hi, d_lo, d_hi = cdf.gather(-1, lo), cdf.gather(-1, hi), d.gather(-1, lo), d.gather(-1, hi)
    den = c_hi - c_lo
    den = torch.where(den < den_min, torch.ones_like(den), den)
    fine = d_lo + (u - c_lo) / den * (d_hi - d_lo)
    return dict(fine=fine, wsum=wsum[:, 0], cdf=cdf)


def coarse_query(rays, num_coarse, num_fine, factors, upsample_inv_s, use_estimate, dtype=torch.float32, radius=RADIUS,
                 forward_inv_s=FORWARD_INV_S):
    """the unperturbed 'multistep_estimate' loop with linear coarse steps on the analytic sphere, every step in `dtype`
    -> (t [R, K-1] mid-points, opacity_alpha [R, K-1]), K = num_coarse + 1 + len(factors) * (num_fine // 2 * 2 + 1)"""
    o, v = rays['rays_o'].cpu().to(dtype), rays['rays_d'].cpu().to(dtype)
    near, far = rays['near'].cpu().to(dtype)[:, None], rays['far'].cpu().to(dtype)[:, None]
    sdf_at = lambda t: (o[:, None, :] + v[:, None, :] * t[..., None]).norm(dim=-1) - radius
    n = num_coarse + 1
    d_all = near + torch.arange(n, dtype=dtype) * ((far - near) / (n - 1))
    sdf_all = sdf_at(d_all)
    m = num_fine // 2 * 2 + 1
    for i, f in enumerate(factors):
        fine = stage(d_all, sdf_all, shared_u(m, dtype), upsample_inv_s * f, use_estimate, dtype)['fine']
        d_all, order = torch.sort(torch.cat([d_all, fine], -1), dim=-1, stable=True)
        if i < len(factors) - 1:
            sdf_all = torch.cat([sdf_all, sdf_at(fine)], -1).gather(-1, order)
    c = torch.sigmoid(sdf_at(d_all) * forward_inv_s)
    alpha = ((c[:, :-1] - c[:, 1:]) / (c[:, :-1] + 1e-5)).clamp_min(0)
    return 0.5 * (d_all[:, 1:] + d_all[:, :-1]), alpha
