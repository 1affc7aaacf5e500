#!/usr/bin/env python
"""tools/exp_embedders.py -- the embedders measured against their torch formulations on one GPU -> profiles/embedders.json.

2^22 rows.  Each case runs in alternated rounds (HIP, torch, HIP, torch, ...), a round is the mean of ITERS launches between two
events after a warm-up, the figure is the median of the rounds.  Cases: SH degree 4 forward and forward + backward (recompute and
stored Jacobian); frequency D = 3 with 10 and 6 frequencies, forward, forward + backward and the eikonal-style double backward.  The
torch side is ``SinusoidalEmbedder`` and, for SH, an UNFUSED torch expression of the same polynomials (monomial sums, coefficients
precomputed outside the timed region).  ``eff`` = algorithmic bytes /
(time * 8 TB/s).

    python tools/exp_embedders.py [--rows 4194304] [--rounds 7] [--iters 10] [--out profiles/embedders.json]
    rocprofv3 --kernel-trace --stats -- python tools/exp_embedders.py --rounds 1 --iters 3 --out /dev/null     # kernel statistics"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK = 8.0e12


def sh_torch_plan(degree=4):
    """per column: ([(power of z, coefficient)], [(binomial coefficient with its sign, power of x, power of y)]), built ONCE outside the
    timed region from the test restatement's closed form"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import embedders_ref as R
    plan = []
    for l in range(degree):
        for m in range(-l, l + 1):
            a = abs(m)
            xy = [(float(math.comb(a, k) * (-1) ** (k // 2)), a - k, k) for k in range(a + 1) if (k % 2 == 0) == (m > 0)] if a else []
            plan.append((R.zpoly(l, a), xy))
    return plan


def sh_torch(p, plan):
    """the same polynomials as a plain torch expression: every column an un-factored sum of monomials, one small kernel per operation
    (what a user without the extension would write; nothing is fused)"""
    x, y, z = p.unbind(-1)
    cols = []
    for zterms, xy in plan:
        q = sum(c * z ** pw for pw, c in zterms)
        if xy:
            q = q * sum(c * x ** px * y ** py for c, px, py in xy)
        cols.append(q if torch.is_tensor(q) else torch.full_like(x, q))
    return torch.stack(cols, -1)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2 ** 22)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embedders.json"))
    args = ap.parse_args()
    from nr3d_lib_amd.models.embedders import FreqEncoder, SHEncoder, get_sinusoidal_embedder
    from nr3d_lib_amd.models.embedders.spherical_harmonics import sphere_harmonics as shmod
    dev = torch.device("cuda:0")
    B = args.rows
    torch.manual_seed(0)
    x = (torch.rand(B, 3, device=dev) * 2 - 1)
    xg = x.clone().requires_grad_(True)
    cases = {}

    def add(name, hip, ref, nbytes):
        cases[name] = (hip, ref, nbytes)

    sh = SHEncoder(3, 4)
    plan = sh_torch_plan(4)
    g16 = torch.randn(B, 16, device=dev)

    def sh_fb(recompute):
        def f():
            shmod.RECOMPUTE_BACKWARD = recompute
            torch.autograd.grad(sh(xg), xg, g16)
        return f

    def sh_fb_torch():
        torch.autograd.grad(sh_torch(xg, plan), xg, g16)

    add("sh4_fwd", lambda: sh(x), lambda: sh_torch(x, plan), B * (12 + 64))
    add("sh4_fwd_bwd_recompute", sh_fb(True), sh_fb_torch, B * (12 + 64) + B * (12 + 64 + 12))
    add("sh4_fwd_bwd_stored", sh_fb(False), sh_fb_torch, B * (12 + 64 + 192) + B * (64 + 192 + 12))
    for n in (10, 6):
        C = 3 + 6 * n
        enc, leg = FreqEncoder(3, n), get_sinusoidal_embedder(n, 3)[0].to(dev)
        g = torch.randn(B, C, device=dev, requires_grad=True)

        def fwd_bwd(e, g=g):
            return lambda: torch.autograd.grad(e(xg), xg, g)

        def eik(e, g=g):
            def f():
                nab, = torch.autograd.grad(e(xg), xg, g, create_graph=True)
                torch.autograd.grad(((nab.norm(dim=-1) - 1) ** 2).mean(), (xg, g))
            return f

        add(f"freq{n}_fwd", lambda enc=enc: enc(x), lambda leg=leg: leg(x), B * (12 + 4 * C))
        add(f"freq{n}_fwd_bwd", fwd_bwd(enc), fwd_bwd(leg), B * (12 + 4 * C) + B * (8 * C + 12))
        add(f"freq{n}_eikonal", eik(enc), eik(leg), B * (12 + 4 * C) + B * (8 * C + 12) + B * (12 + 8 * C + 4 * C + 12))
    res = {"rows": B, "rounds": args.rounds, "iters": args.iters, "device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK, "cases": {}}
    for name, (hip, ref, nbytes) in cases.items():
        th, tr = [], []
        for _ in range(args.rounds):
            th.append(timed(hip, args.iters))
            tr.append(timed(ref, args.iters))
        h, r = statistics.median(th), statistics.median(tr)
        res["cases"][name] = {"hip_ms": round(h, 4), "torch_ms": round(r, 4), "speedup": round(r / h, 3), "algorithmic_bytes": nbytes,
                              "eff": round(nbytes / (h * 1e-3 * PEAK), 4), "hip_rounds_ms": [round(t, 4) for t in th],
                              "torch_rounds_ms": [round(t, 4) for t in tr]}
        print(name, res["cases"][name]["hip_ms"], res["cases"][name]["torch_ms"], res["cases"][name]["speedup"], flush=True)
    shmod.RECOMPUTE_BACKWARD = True
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
