"""The reference's chain for the last stage of a NeuS render (nr3d_lib/models/fields/neus/renderer_mixin.py:396-439), restated in plain
torch ops so that it runs in float64 and in float32 on any device, with its gradients from autograd; and the inputs of the tests.

Rows: ``ray_alpha_to_vw`` literally ((1 + 1e-10) - alpha, shifted, cumprod).  Packs: ``packed_alpha_to_vw`` with ``early_stop_eps``
and ``alpha_thre = 0`` on a padded [P, longest] view of the packs -- the transmittance does not rise, so "stop at the first sample
whose transmittance is below early_stop_eps" is the mask ``T < eps``; a sample with alpha <= 0 has no weight and no effect.  The
generator keeps packed alphas below 1, so the reference backward kernel's ``max(1 - alpha, 1e-10)`` divisor is the plain derivative.
"""
import numpy as np
import torch
import torch.nn.functional as F

EARLY_STOP_EPS = 1e-4
PACK_LENGTHS = (0, 1, 63, 64, 65, 200)
OUTPUTS = ("vw", "mask", "depth", "rgb", "normals")
GRADS = ("g_alpha", "g_t", "g_rgb", "g_nablas")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _nablas(rng, shape):
    """normal vectors with components outside [-1, 1] and some exactly zero vectors"""
    nab = (rng.standard_normal((*shape, 3)) * 1.5).astype(np.float32)
    flat = nab.reshape(-1, 3)
    flat[:: 5] = 0.0
    assert flat.shape[0] < 10 or ((np.abs(nab) > 1).any() and (flat == 0).all(axis=1).any())
    return nab


def _hit(rng, P):
    """shuffled rays_inds_hit into num_rays = P + 3 rays"""
    num_rays = P + 3
    return rng.permutation(num_rays)[:P].astype(np.int64), num_rays


def rows_inputs(R, n, seed=0, kind="random"):
    """kind: "random"; "opaque" -- an exact alpha == 1 at the first (row % 3 == 0), a middle (1) or the last (2) sample; "zero" -- all-zero
    alpha"""
    rng = np.random.default_rng(seed)
    alpha = (rng.random((R, n)) ** 3).astype(np.float32)
    opaque_at = None
    if kind == "opaque":
        opaque_at = np.array([(0, n // 2, n - 1)[r % 3] for r in range(R)])
        alpha[np.arange(R), opaque_at] = 1.0
    elif kind == "zero":
        alpha[:] = 0.0
    t = np.sort(rng.uniform(0.5, 6.0, (R, n)).astype(np.float32), axis=1)
    hit, num_rays = _hit(rng, R)
    return dict(layout="rows", alpha=alpha, t=t, rgb=rng.random((R, n, 3)).astype(np.float32), nablas=_nablas(rng, (R, n)),
                pack_infos=None, rays_inds_hit=hit, num_rays=num_rays, opaque_at=opaque_at, P=R)


def pack_inputs(P, seed=0, margin=True, gaps=True):
    """packs of lengths 0, 1, 63, 64, 65, 200 in turn, a gap of 0-3 samples in front of each, shuffled rays_inds_hit.  Asserted in
    float64: no transmittance lies within a relative 1e-3 of early_stop_eps, so no sample's membership depends on rounding
    (``margin=False`` leaves that out: for comparisons of two kernels with the same arithmetic, bit for bit).  ``gaps=False``: the packs
    tile the buffer, as the pack_infos_hit of a query's volume buffer do."""
    rng = np.random.default_rng(seed)
    lens = np.array([PACK_LENGTHS[p % len(PACK_LENGTHS)] for p in range(P)], dtype=np.int64)
    gaps = rng.integers(0, 4, P) * int(gaps)
    first = np.cumsum(gaps + np.concatenate([[0], lens[:-1]]))
    S = int(first[-1] + lens[-1] + (2 if gaps.any() else 0))
    scale = np.repeat(rng.choice([0.05, 0.3, 0.9], P), lens)
    alpha = np.zeros(S, dtype=np.float32)
    inside = np.concatenate([np.arange(f, f + l) for f, l in zip(first, lens)]) if lens.sum() else np.zeros(0, dtype=np.int64)
    alpha[inside] = (rng.random(inside.size) ** 2 * scale).astype(np.float32)
    for f, l in zip(first, lens):
        T = np.cumprod(np.concatenate([[1.0], 1.0 - alpha[f:f + l].astype(np.float64)]))
        assert not margin or (np.abs(T - EARLY_STOP_EPS) > 1e-3 * EARLY_STOP_EPS).all(), f"pack_inputs(P={P}, seed={seed}): T within 1e-3 of early_stop_eps"
    t = rng.uniform(0.5, 6.0, S).astype(np.float32)
    hit, num_rays = _hit(rng, P)
    return dict(layout="packs", alpha=alpha, t=t, rgb=rng.random((S, 3)).astype(np.float32), nablas=_nablas(rng, (S,)),
                pack_infos=np.stack([first, lens], axis=1).astype(np.int64), rays_inds_hit=hit, num_rays=num_rays, P=P)


def cotangents(inp, seed=1):
    """dL/d(output) for every output, float32"""
    rng = np.random.default_rng(seed)
    nr = inp["num_rays"]
    g = lambda *shape: rng.standard_normal(shape).astype(np.float32)       # noqa: E731
    return dict(vw=g(*inp["alpha"].shape), mask=g(nr), depth=g(nr), rgb=g(nr, 3), normals=g(nr, 3))


# ---- the chain ------------------------------------------------------------------------------------------------------------------
def _padded(pack_infos, device):
    first, lens = pack_infos[:, 0], pack_infos[:, 1]
    longest = int(lens.max()) if lens.numel() else 0
    j = torch.arange(max(longest, 1), device=device)
    valid = j[None, :] < lens[:, None]
    idx = torch.where(valid, first[:, None] + j[None, :], torch.zeros_like(first[:, None]))
    return idx, valid


def composite(alpha, t, rgb, nablas, pack_infos, rays_inds_hit, num_rays, normalize_depth, normalized_normals, scatter=True):
    """-> dict(vw, mask, depth, rgb, normals): the chain on tensors of any float dtype / device; differentiable"""
    if pack_infos is None:
        shifted = torch.roll((1 + 1e-10) - alpha, 1, dims=-1)
        shifted = torch.cat([torch.ones_like(shifted[..., :1]), shifted[..., 1:]], dim=-1)
        w = alpha * torch.cumprod(shifted, dim=-1)
        vw, tt, cc, nn = w, t, rgb, nablas
    else:
        idx, valid = _padded(pack_infos, alpha.device)
        a = torch.where(valid & (alpha[idx] > 0), alpha[idx], torch.zeros_like(alpha[idx]))
        T = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), 1 - a[:, :-1]], dim=1), dim=1)
        w = torch.where(T < EARLY_STOP_EPS, torch.zeros_like(a), a * T)
        vw = torch.zeros_like(alpha).index_put((idx[valid],), w[valid])
        tt = t[idx]
        cc = None if rgb is None else rgb[idx]
        nn = None if nablas is None else nablas[idx]
    mask = w.sum(dim=-1)
    depth = ((w / (mask.unsqueeze(-1) + 1e-10)) * tt).sum(dim=-1) if normalize_depth else (w * tt).sum(dim=-1)
    out = dict(vw=vw, mask=mask, depth=depth, rgb=None, normals=None)
    if rgb is not None:
        out["rgb"] = (w.unsqueeze(-1) * cc).sum(dim=-2)
    if nablas is not None:
        out["normals"] = (w.unsqueeze(-1) * (F.normalize(nn.clamp(-1, 1), dim=-1) if normalized_normals else nn)).sum(dim=-2)
    if scatter and rays_inds_hit is not None:
        for k in ("mask", "depth", "rgb", "normals"):
            if out[k] is not None:
                full = out[k].new_zeros((num_rays, *out[k].shape[1:]))
                out[k] = full.index_put((rays_inds_hit,), out[k])
    return out


def evaluate(inp, dtype, device, with_rgb=True, with_nablas=True, hit=True, normalize_depth=True, normalized_normals=False,
             with_g_vw=True, grads=True):
    """the chain and its gradients (cotangents(inp)) in ``dtype`` on ``device`` -> dict of OUTPUTS and GRADS (None where not asked for)"""
    to = lambda a, dt=dtype: None if a is None else torch.as_tensor(a).to(device=device, dtype=dt)      # noqa: E731
    need = grads and not normalized_normals
    leaf = lambda a: to(a).requires_grad_(need)         # noqa: E731
    alpha, t = leaf(inp["alpha"]), leaf(inp["t"])
    rgb = leaf(inp["rgb"]) if with_rgb else None
    nablas = leaf(inp["nablas"]) if with_nablas else None
    P = inp["P"]
    out = composite(alpha, t, rgb, nablas, to(inp["pack_infos"], torch.int64), to(inp["rays_inds_hit"], torch.int64) if hit else None,
                    inp["num_rays"] if hit else P, normalize_depth, normalized_normals)
    res = {k: (None if v is None else v.detach()) for k, v in out.items()}
    res.update({k: None for k in GRADS})
    if need:
        cot = cotangents(inp)
        loss = 0
        for k in OUTPUTS:
            if out[k] is not None and (k != "vw" or with_g_vw):
                g = to(cot[k])
                loss = loss + (out[k] * (g if (hit or k == "vw") else g[:P])).sum()
        wrt = [(k, x) for k, x in zip(GRADS, (alpha, t, rgb, nablas)) if x is not None]
        got = torch.autograd.grad(loss, [x for _, x in wrt], allow_unused=True)
        for (k, x), g in zip(wrt, got):
            res[k] = torch.zeros_like(x) if g is None else g
    return res
