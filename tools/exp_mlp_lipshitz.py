#!/usr/bin/env python
"""tools/exp_mlp_lipshitz.py -- LipshitzMLP with the one-launch weight normalisation (models.blocks.mlp.FUSED_LIPSHITZ) measured on one
GPU -> profiles/mlp_lipschitz.json.

The fused route (normalisation in one launch each way, the layers on the fused decoder kernels) against the switch off (the reference's
torch chain, layer by layer; same library, same process) on this package's own ``LipshitzMLP`` 35 -> 64 -> 64 -> 3, ReLU hidden layers and
a sigmoid output, as an fp32 and as a half block, at 2^12 samples (launch bound: where the normalisation shows) and 2^22; forward (no
grad) and forward + backward (x and every parameter ask for a gradient).  The plain ``MLP`` of the same shape runs in the same rounds: the
difference to it is the cost of being Lipschitz.  The bounds sit at half the layers' inf-norms, so rows are scaled.  A round is the mean
of ITERS calls between two events after a warm-up, ITERS (the same for all routes) chosen per case so that the fused route's round lasts
about a quarter of a second; the routes alternate, the figure is the median of the rounds.  ``abi``: the two new entries alone, called at
the C ABI on the same three weight matrices.  ``default_supported``: the fused route is faster in every row by more than the spread of
its own and the chain's rounds -- what FUSED_LIPSHITZ's default has to follow.

    python tools/exp_mlp_lipshitz.py [--rounds 7] [--out profiles/mlp_lipschitz.json]
    python tools/exp_mlp_lipshitz.py --yardstick LOG   # fold the "YARDSTICK ..." lines of a `pytest -s tests/test_mlp_lipschitz_gpu.py` log into the JSON

Launches of the normalisation per direction, from the profiler and not from a count of the code (a run of its own, no counters):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o lip -- python tools/exp_mlp_lipshitz.py --trace
    python tools/exp_mlp_lipshitz.py --read-trace DIR  # no GPU needed: splits DIR's kernel trace at the marker kernel, adds "launches"
``--trace`` runs TRACE_ITERS calls of each of the four phases (fused | chain) x (forward | backward) of the normalisation of the three
layers alone, with one launch of a marker kernel (k_tau_to_alpha_fwd, which neither route uses) in front of each phase and behind the last."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "mlp_lipschitz.json")
DIMS = (35, 64, 64, 3)
SAMPLES = (1 << 12, 1 << 22)
TRACE_ITERS = 10
WINDOW_MS = 250.0
TRACE_PHASES = ("fused forward", "fused backward", "chain forward", "chain backward")
MARKER = "k_tau_to_alpha_fwd"


def merge_into(path, **sections):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res.update(sections)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def read_yardstick(log, out):
    """the figures the GPU tests printed: per quantity the count, the largest and the median ratio to torch's own fp32 error"""
    by, bounds = {}, {}
    for line in open(log):
        m = re.search(r"YARDSTICK (.*?): .*ratio ([0-9.infa]+)", line)
        if m and m.group(2) not in ("inf", "nan"):
            what = m.group(1).split("[")[0].strip()
            by.setdefault(what, []).append((float(m.group(2)), m.group(1)))
        m = re.search(r"YARDSTICK (W~.*?): largest error / bound ([0-9.e+-]+)", line)
        if m:
            bounds[m.group(1)] = float(m.group(2))
    merge_into(out, yardstick_note="ratio = error against float64 / the same error of torch's fp32 chain on the same inputs and device; the "
                                   "bounds are 8 (kernels, eikonal step) and 4 (first order end to end), see tests/test_mlp_lipschitz_gpu.py",
               yardstick={k: {"checks": len(v), "largest_ratio": max(v)[0], "at": max(v)[1],
                              "median_ratio": round(statistics.median(r for r, _ in v), 3)} for k, v in sorted(by.items())},
               forward_error_over_bound=bounds)
    print({k: (len(v), max(v)[0]) for k, v in by.items()})


def read_trace(trace_dir, out):
    f = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    cuts = [i for i, r in enumerate(rows) if MARKER in r["Kernel_Name"]]
    assert len(cuts) == len(TRACE_PHASES) + 1, f"{len(cuts)} marker launches in {f}"
    launches = {}
    for phase, a, b in zip(TRACE_PHASES, cuts[:-1], cuts[1:]):
        names = [r["Kernel_Name"] for r in rows[a + 1:b]]
        per = {}
        for n in names:
            per[n[:100]] = per.get(n[:100], 0) + 1
        launches[phase] = {"per_call": len(names) / TRACE_ITERS, "kernels": {k: v / TRACE_ITERS for k, v in sorted(per.items())}}
    merge_into(out, launches=dict(source="rocprofv3 --kernel-trace --stats, a run of its own; the normalisation of the three layers of "
                                         "35 -> 64 -> 64 -> 3 alone; backward = the backward pass alone", iters=TRACE_ITERS, **launches))
    print({k: v["per_call"] for k, v in launches.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--read-trace", default=None)
    ap.add_argument("--yardstick", default=None)
    args = ap.parse_args()
    if args.read_trace:
        return read_trace(args.read_trace, args.out)
    if args.yardstick:
        return read_yardstick(args.yardstick, args.out)

    import torch
    from nr3d_lib_amd import _hip as H
    from nr3d_lib_amd.bindings import _mlp, _pack_ops
    from nr3d_lib_amd.models.blocks import MLP, LipshitzMLP
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")

    def net(cls, dtype):
        torch.manual_seed(0)
        m = cls(DIMS[0], DIMS[-1], D=len(DIMS) - 2, W=list(DIMS[1:-1]), activation="relu", output_activation="sigmoid", dtype=dtype, device=dev)
        if cls is LipshitzMLP:
            with torch.no_grad():
                m.lipshitz_bound_per_layer.copy_(m.initial_bounds(0.5))
        return m

    def calls(m, x0, gy, fused):
        """(forward without grad, forward + backward) of one route"""
        x = x0.clone().requires_grad_(True)

        def forward():
            mlp_mod.FUSED_LIPSHITZ = fused
            with torch.no_grad():
                return m(x0)

        def both():
            mlp_mod.FUSED_LIPSHITZ = fused
            x.grad = None
            m.zero_grad(set_to_none=True)
            m(x).backward(gy)

        return forward, both

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

    def alternated(fns, iters):
        ts = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                ts[k].append(timed(fn, iters))
        r = {}
        for k, v in ts.items():
            r[k + "_ms"] = round(statistics.median(v), 4)
            r[k + "_rounds_ms"] = [round(t, 4) for t in v]
        r["speedup"] = round(r["chain_ms"] / r["fused_ms"], 3)
        r["fused_over_plain"] = round(r["fused_ms"] / r["plain_ms"], 3)
        # faster by more than the spread of the rounds: the slowest fused round still beats the fastest chain round
        r["faster_beyond_spread"] = max(ts["fused"]) < min(ts["chain"])
        return r

    def normalisation_phases(m):
        """the normalisation of all layers alone: (forward, backward) per route, for the trace"""
        c, ws = m.lipshitz_bound_per_layer, [l.weight for l in m.layers]
        gs = [torch.randn_like(w) for w in ws]
        phases = []
        for fused in (True, False):
            def forward(fused=fused):
                if fused:
                    return list(mlp_mod.LipschitzNormalizeFunction.apply(c, *ws))
                return [m.normalization(w, torch.nn.functional.softplus(c[i])) for i, w in enumerate(ws)]
            kept = forward()

            def backward(kept=kept):
                return torch.autograd.grad(kept, [c, *ws], gs, retain_graph=True)
            phases += [forward, backward]
        return phases

    saved = mlp_mod.FUSED_LIPSHITZ
    try:
        if args.trace:
            phases = normalisation_phases(net(LipshitzMLP, torch.float))
            sigma = torch.rand(64, device=dev)
            for fn in phases:                                  # code objects loaded, allocator warm
                fn()
            torch.cuda.synchronize()
            for fn in phases:
                _pack_ops.tau_to_alpha_forward(sigma, sigma)
                for _ in range(TRACE_ITERS):
                    fn()
            _pack_ops.tau_to_alpha_forward(sigma, sigma)
            torch.cuda.synchronize()
            return
        res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "dims": list(DIMS), "blocks": {}}
        gen = torch.Generator().manual_seed(0)
        for tag, dtype in (("fp32", torch.float), ("half", torch.half)):
            lip, plain = net(LipshitzMLP, dtype), net(MLP, dtype)
            for n in SAMPLES:
                x0 = torch.randn(n, DIMS[0], generator=gen).to(dev)
                gy = torch.randn(n, DIMS[-1], generator=gen).to(dev).to(dtype)
                f_fwd, f_both = calls(lip, x0, gy, True)
                c_fwd, c_both = calls(lip, x0, gy, False)
                p_fwd, p_both = calls(plain, x0, gy, True)
                a_f, a_c = f_fwd().float(), c_fwd().float()
                iters = {k: max(20, int(WINDOW_MS / timed(fn, 10))) for k, fn in (("forward", f_fwd), ("forward_backward", f_both))}
                r = {"samples": n, "iters": iters, "max_abs_y_difference": (a_f - a_c).abs().max().item(),
                     "forward": alternated(dict(fused=f_fwd, chain=c_fwd, plain=p_fwd), iters["forward"]),
                     "forward_backward": alternated(dict(fused=f_both, chain=c_both, plain=p_both), iters["forward_backward"])}
                res["blocks"][f"{tag} n=2^{n.bit_length() - 1}"] = r
                print(tag, n, "forward", r["forward"]["fused_ms"], r["forward"]["chain_ms"], r["forward"]["plain_ms"], "forward + backward",
                      r["forward_backward"]["fused_ms"], r["forward_backward"]["chain_ms"], r["forward_backward"]["plain_ms"], flush=True)
                del x0, gy
        # the two entries alone, at the C ABI: argument arrays built once, nothing of the binding's checks or allocations in the loop
        m = net(LipshitzMLP, torch.float)
        ws = [l.weight.detach() for l in m.layers]
        c = m.lipshitz_bound_per_layer.detach()
        gs, outs, dws, dc = [torch.randn_like(w) for w in ws], [torch.empty_like(w) for w in ws], [torch.empty_like(w) for w in ws], torch.empty_like(c)
        rows, cols = (C.c_uint32 * 3)(*[w.shape[0] for w in ws]), (C.c_uint32 * 3)(*[w.shape[1] for w in ws])
        pw, po, pg, pd = (_mlp._ptr_array(t) for t in (ws, outs, gs, dws))
        lib, st = H.lib(), H.stream_of(c)

        def abi_fwd():
            H.check(lib.nr3d_mlp_lipschitz_normalize(3, rows, cols, pw, 0, H.ptr(c), po, st))

        def abi_bwd():
            H.check(lib.nr3d_mlp_lipschitz_normalize_backward(3, rows, cols, pw, 0, H.ptr(c), pg, pd, H.ptr(dc), st))

        res["abi"] = {}
        for k, fn in (("normalize", abi_fwd), ("normalize_backward", abi_bwd)):
            iters = max(200, int(WINDOW_MS / timed(fn, 200)))
            v = [timed(fn, iters) for _ in range(args.rounds)]
            res["abi"][k] = {"ms": round(statistics.median(v), 5), "iters": iters, "rounds_ms": [round(t, 5) for t in v]}
            print("abi", k, res["abi"][k]["ms"], flush=True)
        res["default_supported"] = all(r[k]["faster_beyond_spread"] for r in res["blocks"].values() for k in ("forward", "forward_backward"))
        print("fused faster in every row by more than the spread:", res["default_supported"], flush=True)
        merge_into(args.out, **res)
    finally:
        mlp_mod.FUSED_LIPSHITZ = saved


if __name__ == "__main__":
    main()
