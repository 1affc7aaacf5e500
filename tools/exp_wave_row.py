#!/usr/bin/env python
"""tools/exp_wave_row.py [OUT] -- one SHA-256 per output tensor of every entry whose kernel is built from csrc/wave_row.h, on seeded inputs
-> OUT (default: standard output only).

The building blocks of the ray-stage kernels (wave scans, the running maximum, the merge-path search) are stated once in wave_row.h;
moving code there must not change one output bit.  The entries around them (inverse CDF, clipped packs, composites) are covered too.  This file calls the bindings only, so the same
file runs against two trees: run it in each, in a process of its own, and compare the two printouts line for line
(profiles/wave_row_digests.txt holds them side by side).  A difference is no tolerance question: an expression was reordered.

Shapes, the smallest at which each block can go wrong: row and pack lengths 1, 2, 63, 64, 65, 130 (the chunk carry of the scans and of
the running maximum); m in 1, 9, 65; per packed stage one pack that just fits the LDS row and one that just does not (the row is asked of
the library); u shared and per row; depth ties between old and new samples (repeated depths, whose empty bins return an old depth, u = 0
and u = 1, and for packed_invert_cdf u on the CDF's own values), which is where the two tie rules of the merge differ.  The forced
positions (0, 1, a repeated u) go into the rows of m = 9 and m = 65 only: m = 1 exercises no forced tie.  In merge_rows_packs a tie
is forced on every fourth ray, where the first coarse depth is set to the pack's first marched one."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LENGTHS = (1, 2, 63, 64, 65, 130)
MS = (1, 9, 65)


def main():
    import torch
    from nr3d_lib_amd import _hip
    from nr3d_lib_amd.bindings import _nerf_upsample, _neus_composite, _neus_upsample, _pack_ops
    assert torch.cuda.is_available(), "the digests are of what the GPU computes"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = []

    def digest(name, *tensors):
        for i, t in enumerate(tensors):
            h = "none" if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
            lines.append(f"{name} [{i}] {h}")

    def rand(*shape):
        return torch.rand(*shape, generator=gen)

    def depths(n, ties):
        """n sorted depths in [0.5, 3.5); with `ties` every third one repeats its predecessor (a span of length zero)"""
        d = (0.5 + 3.0 * rand(n)).sort().values
        if ties and n > 1:
            i = torch.arange(1, n, 3)
            d[i] = d[i - 1]
        return d

    def positions(rows, m, shared):
        """non-decreasing CDF positions with 0, 1 and a repeated value among them"""
        u = rand(1 if shared else rows, m).sort(-1).values
        if m >= 9:
            u[:, 0], u[:, -1], u[:, 4] = 0.0, 1.0, u[:, 3]
        return (u[0] if shared else u).contiguous().to(dev)

    def packs(lens):
        lens = torch.tensor(lens, dtype=torch.int64)
        return torch.stack([lens.cumsum(0) - lens, lens], 1).contiguous()

    def packed_depths(pi):
        return torch.cat([depths(int(n), p % 2 == 1) for p, n in enumerate(pi[:, 1])] + [torch.zeros(0)])

    def sdf_of(d):
        return (2.0 - d + 0.05 * torch.randn(d.shape, generator=gen)).contiguous()

    # ---- _neus_upsample.upsample_stage: rows (n >= 2) ----
    for n in LENGTHS[1:]:
        d = torch.stack([depths(n, r % 2 == 1) for r in range(7)])
        s = sdf_of(d)
        for m in MS:
            for shared in (True, False):
                u = positions(7, m, shared)
                for est in (False, True):
                    digest(f"neus rows n={n} m={m} shared={int(shared)} est={int(est)}",
                           *_neus_upsample.upsample_stage(d.to(dev), s.to(dev), u, 16.0, est))

    # ---- _neus_upsample.upsample_stage_packed ----
    row = _neus_upsample.PACKED_LDS_ROW
    for m in MS:
        pi = packs(list(LENGTHS) * 8 + [row - m, row - m + 1])
        d = packed_depths(pi)
        s = sdf_of(d)
        for shared in (True, False):
            u = positions(pi.shape[0], m, shared)
            for est in (False, True):
                for merge, need_sdf in ((True, True), (True, False), (False, False)):
                    out = _neus_upsample.upsample_stage_packed(d.to(dev), s.to(dev), pi.to(dev), u, 16.0, est, merge=merge, need_sdf=need_sdf)
                    if out[2] is not None:
                        out[2][out[3].flatten()] = 0.0        # the places of the new depths are the caller's to fill
                    digest(f"neus packs m={m} shared={int(shared)} est={int(est)} merge={int(merge)} sdf={int(need_sdf)}", *out)

    # ---- _nerf_upsample.merge_rows_packs: a missed ray (length 0) first, last and in between ----
    row = _nerf_upsample.LDS_ROW
    for nc in (1, 9, 64):
        pi = packs([0] + list(LENGTHS) * 8 + [0, row - nc, row - nc + 1, 0])
        R = pi.shape[0]
        d = packed_depths(pi)
        coarse = torch.stack([depths(nc, r % 3 == 1) for r in range(R)])
        first = pi[:, 0].clamp(max=max(d.shape[0] - 1, 0))
        coarse[1::4, 0] = d[first[1::4]]                      # a coarse depth on a marched one, where the pack has one
        coarse = coarse.sort(-1).values.contiguous()
        o, dr = torch.randn(R, 3, generator=gen), torch.randn(R, 3, generator=gen)
        digest(f"nerf merge nc={nc}", *_nerf_upsample.merge_rows_packs(coarse.to(dev), d.to(dev), pi.to(dev), o.to(dev), dr.to(dev)))

    # ---- _nerf_upsample.upsample_stage_packed, with and without the coarse rows ----
    for m in MS:
        for nc in (0, 9):
            pi = packs(list(LENGTHS) * 8 + [row - m - nc, row - m - nc + 1])
            P = pi.shape[0]
            d = packed_depths(pi)
            sigma, delta = (4.0 * rand(d.shape[0]) ** 2).to(dev), (0.05 * rand(d.shape[0])).to(dev)
            coarse = torch.stack([depths(nc, p % 3 == 1) for p in range(P)]).contiguous().to(dev) if nc else None
            for shared in (True, False):
                u = positions(P, m, shared)
                digest(f"nerf packs m={m} nc={nc} shared={int(shared)}",
                       *_nerf_upsample.upsample_stage_packed(d.to(dev), sigma, delta, pi.to(dev), u, coarse=coarse))

    # ---- packed_invert_cdf: positions on the CDF's own values, below its first and at its last ----
    pi = packs(list(LENGTHS) * 8)
    d = packed_depths(pi)
    weights = [torch.cat([rand(1) + 1e-3, (rand(int(n)) * (rand(int(n)) > 0.3))[1:]]) for n in pi[:, 1]]      # empty bins among them
    cdf = torch.cat([w.cumsum(0) / w.sum() for w in weights])
    for m in MS:
        u = rand(pi.shape[0], m)
        if m >= 9:
            for p, (b, n) in enumerate(pi.tolist()):
                u[p, 0], u[p, 1], u[p, 2], u[p, 3] = 0.0, 1.0, cdf[b + n // 2], cdf[b + n - 1]
        digest(f"invert_cdf m={m}", *_pack_ops.packed_invert_cdf(d.to(dev), cdf.contiguous().to(dev), u.contiguous().to(dev), pi.to(dev)))

    # ---- packed_alpha_to_vw and the fused composite at pack_scan = 1; the NeuS composite on packs and rows ----
    _hip.set_option("pack_scan", 1)
    try:
        P, S = pi.shape[0], d.shape[0]
        alphas = rand(S) ** 3
        alphas[::17], alphas[5::29] = 0.0, 1.0
        alphas, t, rgb, nablas = alphas.to(dev), d.to(dev), rand(S, 3).to(dev), torch.randn(S, 3, generator=gen).to(dev)
        pid = pi.to(dev)
        digest("alpha_to_vw", _pack_ops.packed_alpha_to_vw_forward(alphas, pid, 1e-4, 0.0, False)[0])
        g = [torch.randn(*s, generator=gen).to(dev) for s in ((P,), (P,), (P, 3), (P, 3), (S,))]
        vw, mask, depth, rgb_out = _pack_ops.packed_composite_forward(alphas, t, rgb, pid, None, P, 1e-4, 0.0, True)
        digest("composite fwd", vw, mask, depth, rgb_out)
        digest("composite bwd", *_pack_ops.packed_composite_backward(alphas, vw, t, rgb, pid, None, 1e-4, 0.0, True, mask, depth, g[0], g[1],
                                                                      g[2], g[4]))
        out = _neus_composite.neus_composite_forward(alphas, t, rgb, nablas, pack_infos=pid)
        digest("neus composite packs fwd", *out)
        digest("neus composite packs bwd", *_neus_composite.neus_composite_backward(alphas, t, rgb, nablas, pid, None, 1e-4, 0.0, True, 0, out[0],
                                                                                     out[1], out[2], *g))
        for n in LENGTHS:
            R = 5
            a = rand(R, n) ** 3
            a[:, ::7] = 0.0
            a[1, n // 2] = 1.0
            a, t, rgb, nablas = a.to(dev), rand(R, n).to(dev), rand(R, n, 3).to(dev), torch.randn(R, n, 3, generator=gen).to(dev)
            g = [torch.randn(*s, generator=gen).to(dev) for s in ((R,), (R,), (R, 3), (R, 3), (R, n))]
            out = _neus_composite.neus_composite_forward(a, t, rgb, nablas)
            digest(f"neus composite rows n={n} fwd", *out)
            digest(f"neus composite rows n={n} bwd", *_neus_composite.neus_composite_backward(a, t, rgb, nablas, None, None, 1e-4, 0.0, True, 0,
                                                                                             out[0], out[1], out[2], *g))
    finally:
        _hip.set_option("pack_scan", -1)
    torch.cuda.synchronize()

    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
