"""Restatement of the NeuS opacity chain (graphics/neus/neus_utils.py: sdf * inv_s -> sigmoid -> diff | packed_diff -> negate ->
+ 1e-5 -> divide -> clamp_min) in plain torch ops of a chosen dtype, on whatever device its inputs are on: the packed difference is
done by indexing, so no HIP kernel runs.  Shared by tests/test_neus_alpha_cpu.py, tests/test_neus_alpha_gpu.py and
tools/exp_neus_alpha.py: float64 is the reference, float32 torch's own evaluation that the yardstick compares the kernel with."""
import torch

LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 5, 64]          # 1051 samples: one, around one and two waves' strides, a long one
KINDS = ("cross", "noisy", "flat")
INV_S = (20.0, 256.0, 2048.0)


def segment(kind, n, gen):
    """one pack's or row's SDF values: "cross" 0.6 - t, "noisy" 0.3 - 0.6 t + 0.05 randn, "flat" 0.01 | -0.02 (exact ties)"""
    t = torch.linspace(0, 1, n) if n > 1 else torch.zeros(1)
    if kind == "cross":
        return 0.6 - t
    if kind == "noisy":
        return 0.3 - 0.6 * t + 0.05 * torch.randn(n, generator=gen)
    assert kind == "flat"
    return torch.cat([torch.full((n // 2,), 0.01), torch.full((n - n // 2,), -0.02)])


def packs(kind, seed, lengths=LENGTHS, layout="contiguous"):
    """-> (sdf [S], pack_infos int64 [P, 2], appends [P], g [S]) on the CPU.  layout: "contiguous" -- the packs tile [0, S);
    "gaps" -- rows outside every pack in front of, between and behind the packs, and a zero-length pack; "shuffled" -- the gapped
    layout with the packs listed in another order (not ordered: the unordered route)"""
    gen = torch.Generator().manual_seed(seed)
    segs = [segment(kind, n, gen) for n in lengths]
    if layout == "contiguous":
        first, pos = [], 0
        for n in lengths:
            first.append(pos)
            pos += n
        lens, total = list(lengths), pos
    else:
        first, lens, pos = [], [], 3                          # three rows in front of the first pack
        for j, n in enumerate(lengths):
            if j == 4:                                        # a zero-length pack in the middle of the table
                first.append(pos)
                lens.append(0)
            first.append(pos)
            lens.append(n)
            pos += n + (j % 3) * 2                            # gaps of 0, 2, 4 rows
        total = pos + 5                                       # five rows behind the last pack
        segs.insert(4, torch.zeros(0))
    sdf = 0.1 * torch.randn(total, generator=gen)             # rows outside the packs hold values nobody may read into a result
    for b, s in zip(first, segs):
        sdf[b:b + s.numel()] = s
    pack_infos = torch.tensor(list(zip(first, lens)), dtype=torch.int64).reshape(-1, 2)
    if layout == "shuffled":
        pack_infos = pack_infos[torch.randperm(pack_infos.shape[0], generator=gen)].contiguous()
    appends = -0.05 + 0.05 * torch.randn(pack_infos.shape[0], generator=gen)
    g = torch.randn(total, generator=gen)
    return sdf.float(), pack_infos, appends.float(), g.float()


def rows(kind, seed, R, n):
    """-> (sdf [R, n], g [R, n]) on the CPU (g's last column is unused without append)"""
    gen = torch.Generator().manual_seed(seed)
    sdf = torch.stack([segment(kind, n, gen) for _ in range(R)])
    return sdf.float(), torch.randn(R, n, generator=gen).float()


def row_pack_infos(R, n, device):
    return torch.stack([torch.arange(R, device=device) * n, torch.full((R,), n, device=device)], 1).long().contiguous()


def _next_index(pack_infos, S, has_append):
    """per sample: the index of its c_next in cat([cdf [S], appended cdf [P]]), and whether it closes an interval at all"""
    dev = pack_infos.device
    nxt = torch.zeros(S, dtype=torch.long, device=dev)
    valid = torch.zeros(S, dtype=torch.bool, device=dev)
    first, lens = pack_infos[:, 0], pack_infos[:, 1]
    P = pack_infos.shape[0]
    pid = torch.repeat_interleave(torch.arange(P, device=dev), lens)
    offs = torch.arange(pid.numel(), device=dev) - torch.repeat_interleave(lens.cumsum(0) - lens, lens)
    idx = first[pid] + offs                                   # every sample that is in a pack
    last = offs == lens[pid] - 1
    nxt[idx] = torch.where(last, S + pid, idx + 1)
    valid[idx] = ~last | has_append
    return nxt, valid


def _sigmoid64(z):
    """sigmoid for the float64 reference, written so that autograd's derivative is E / (1 + E)^2 with E = exp(-|z|).  torch.sigmoid's
    own derivative y (1 - y) is exactly 0 in float64 from z = 36.8 on (y rounds to 1), while the true c' there -- 1e-16 down to
    float32's smallest numbers -- is what a whole gradient tensor consists of when every sample of it is far from the surface (rows
    of two samples at inv_s 256: all of dL/dsdf is below 2e-25, and entries with z = 49 carry it).  A reference has to be more
    accurate than what it judges.  Same values as torch.sigmoid to the last bits everywhere else."""
    e = torch.exp(torch.where(z >= 0, -z, z))              # not -|z|: autograd's |z|' is 0 at z = 0, a sample on the surface
    return torch.where(z >= 0, 1 / (1 + e), e / (1 + e))


def chain(sdf, inv_s, g=None, pack_infos=None, append_cdf_1=False, appends=None, dtype=torch.float64):
    """the chain in ``dtype``: float32 is torch's own chain, torch.sigmoid included (what the yardstick compares the kernel with);
    float64, the reference, evaluates the sigmoid as ``_sigmoid64``.  Packed: sdf [S], pack_infos [P, 2]; rows (pack_infos None): sdf [..., n] -> alpha [..., n - 1] or
    [..., n].  inv_s: a number or a one-element tensor.  -> dict(alpha) and, with g = dL/dalpha, through autograd g_sdf, g_appends
    (None without appends), g_inv_s, and T = the float64 sum of the absolute un-cancelled contributions to dL/dinv_s:
    sum_i |g_i| (|d alpha_i / d c_i| |c'_i sdf_i| + |d alpha_i / d c_next| |c'_next sdf_next|)."""
    shape = sdf.shape
    dev = sdf.device
    if pack_infos is None:
        n = shape[-1]
        R = sdf.numel() // n
        pack_infos, is_rows = row_pack_infos(R, n, dev), True
    else:
        is_rows = False
    if append_cdf_1:
        appends = None
    S, P = sdf.numel(), pack_infos.shape[0]
    has_append = append_cdf_1 or appends is not None
    x = sdf.detach().reshape(-1).to(dtype).requires_grad_(True)
    s = torch.as_tensor(inv_s).detach().to(device=dev, dtype=dtype).reshape(()).requires_grad_(True)
    a = None if appends is None else appends.detach().to(dtype).requires_grad_(True)
    nxt, valid = _next_index(pack_infos, S, has_append)
    sigmoid = _sigmoid64 if dtype == torch.float64 else torch.sigmoid
    cdf = sigmoid(x * s)
    if append_cdf_1:
        tail = cdf.new_ones(P)
    elif a is not None:
        tail = sigmoid(a * s)
    else:
        tail = cdf.new_zeros(P)
    c_next = torch.cat([cdf, tail])[nxt]
    drop = torch.where(valid, -(c_next - cdf), torch.zeros_like(cdf))
    alpha = (drop / (cdf + 1e-5)).clamp_min(0)
    out_alpha = alpha
    if is_rows:
        out_alpha = alpha.reshape(*shape)
        if not append_cdf_1:
            out_alpha = out_alpha[..., :-1]
    res = dict(alpha=out_alpha.detach())
    if g is None:
        return res
    gg = g.detach().to(dtype)
    if is_rows and not append_cdf_1:
        gg = gg.reshape(-1, shape[-1])[:, :shape[-1] - 1]
    wrt = [x, s] + ([a] if a is not None else [])
    grads = torch.autograd.grad(out_alpha, wrt, gg.reshape(out_alpha.shape))
    res["g_sdf"], res["g_inv_s"] = grads[0].reshape(shape), grads[1]
    res["g_appends"] = grads[2] if a is not None else None
    # T in float64, whatever dtype the chain ran in
    with torch.no_grad():
        x64, s64 = sdf.detach().reshape(-1).double(), float(torch.as_tensor(inv_s).detach().double().reshape(()))
        c = _sigmoid64(x64 * s64)
        dc = torch.exp(-(x64 * s64).abs()) * torch.maximum(c, 1 - c) ** 2          # E / (1 + E)^2
        if append_cdf_1:
            c_t, dc_t, x_t = c.new_ones(P), c.new_zeros(P), c.new_zeros(P)
        elif appends is not None:
            x_t = appends.detach().double()
            c_t = _sigmoid64(x_t * s64)
            dc_t = torch.exp(-(x_t * s64).abs()) * torch.maximum(c_t, 1 - c_t) ** 2
        else:
            c_t, dc_t, x_t = c.new_zeros(P), c.new_zeros(P), c.new_zeros(P)
        cn, dcn, xn = torch.cat([c, c_t])[nxt], torch.cat([dc, dc_t])[nxt], torch.cat([x64, x_t])[nxt]
        den = c + 1e-5
        m = (valid & ((c - cn) / den >= 0)).double()
        g_full = torch.zeros(S, dtype=torch.float64, device=dev)
        if is_rows and not append_cdf_1:
            g_full.reshape(-1, shape[-1])[:, :shape[-1] - 1] = gg.double().reshape(-1, shape[-1] - 1)
        else:
            g_full = gg.double().reshape(-1)
        res["T"] = float((g_full.abs() * m * ((cn + 1e-5) / den ** 2 * (dc * x64).abs() + 1 / den * (dcn * xn).abs())).sum())
    return res


def near_ties(sdf, inv_s, pack_infos=None, appends=None):
    """the number of intervals with 0 < |z_i - z_next| < 1e-4 in float64, z = sdf * inv_s (the interval to the appended value
    included): so close to a tie, float32 and float64 may take different sides of the clamp.  The tests assert 0 on their inputs."""
    if pack_infos is None:
        pack_infos = row_pack_infos(sdf.numel() // sdf.shape[-1], sdf.shape[-1], sdf.device)
    z = sdf.detach().reshape(-1).double() * float(inv_s)
    P = pack_infos.shape[0]
    nxt, valid = _next_index(pack_infos, z.numel(), appends is not None)
    tail = z.new_zeros(P) if appends is None else appends.detach().double() * float(inv_s)
    d = (z - torch.cat([z, tail])[nxt]).abs()
    return int((valid & (d > 0) & (d < 1e-4)).sum())
