#!/usr/bin/env python
"""tools/exp_neus_alpha.py -- the fused NeuS opacity (neus_utils.FUSED_SDF_TO_ALPHA) measured on one GPU -> profiles/neus_alpha.json.

The fused route (one launch each way, bindings._neus_alpha) against the reference's op chain (the switch off: the code path of the
commit before, same library, same process) on the same inputs: rows at 4096 x 64 and 65 536 x 64; packs at 4096 and 65 536 packs of
about 30 and about 300 samples (lengths uniform in [len / 2, 3 len / 2], tiling the buffer and marked ordered, as a marcher's).
Forward, and forward + backward, both with a learnable inv_s on the GPU.  A round is the mean of ITERS calls between two events after
a warm-up, ITERS (the same for both routes) chosen per case so that the fused route's round lasts about a quarter of a second; the two
routes alternate, the figure is the median of the rounds.  ``default_supported``: the fused route is not slower in
any row -- what FUSED_SDF_TO_ALPHA's default has to follow.

    python tools/exp_neus_alpha.py [--rounds 7] [--out profiles/neus_alpha.json]
    python tools/exp_neus_alpha.py --yardstick LOG     # fold the "YARDSTICK ..." lines of a `pytest -s tests/test_neus_alpha_gpu.py` log into the JSON

Launches per direction, from the profiler and not from a count of the code (a run of its own, no counters):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o alpha -- python tools/exp_neus_alpha.py --trace
    python tools/exp_neus_alpha.py --read-trace DIR    # no GPU needed: splits DIR's kernel trace at the marker kernel, adds "launches"
``--trace`` runs, on 4096 packs of about 30, TRACE_ITERS calls of each of the four phases (fused | chain) x (forward | backward) with
one launch of a marker kernel (k_tau_to_alpha_fwd, which neither route uses) in front of each phase and behind the last."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "neus_alpha.json")
ROWS = ((4096, 64), (65536, 64))
PACKS = ((4096, 30), (4096, 300), (65536, 30), (65536, 300))
INV_S = 256.0
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
    """the ratios the GPU tests printed: the count, the largest and the median per quantity"""
    by = {}
    for line in open(log):
        m = re.search(r"YARDSTICK (.*?): .*ratio ([0-9.infa]+)", line)
        if m and m.group(2) not in ("inf", "nan"):
            what = next((k for k in ("dL/dinv_s", "dL/dsdf", "dL/dappends", "dL/dradius", "alpha", "sdf.grad") if k in m.group(1)), "other")
            by.setdefault(what, []).append((float(m.group(2)), m.group(1)))
    merge_into(out, yardstick_note="ratio = error / (torch fp32 chain's error, or for dL/dinv_s the larger of that and eps32 T); the bound is 4, "
                                   "and for the tensors a ratio above it passes while the error is below 1e-5 of the tensor's maximum",
               yardstick={k: {"checks": len(v), "largest_ratio": max(v)[0], "at": max(v)[1],
                                   "median_ratio": round(statistics.median(r for r, _ in v), 3)} for k, v in sorted(by.items())})
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
    merge_into(out, launches=dict(source="rocprofv3 --kernel-trace --stats, a run of its own; 4096 packs of about 30, learnable inv_s; "
                                         "backward = the backward pass alone", iters=TRACE_ITERS, **launches))
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
    from nr3d_lib_amd import _hip
    from nr3d_lib_amd.bindings import _pack_ops
    from nr3d_lib_amd.graphics.neus import neus_utils as nu
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)

    def row_case(R, n):
        t = torch.linspace(0, 1, n)
        sdf = (0.3 - 0.6 * t + 0.05 * torch.randn(R, n, generator=gen)).to(dev)
        return dict(sdf=sdf, g=torch.randn(R, n - 1, generator=gen).to(dev), pack_infos=None)

    def pack_case(P, mean):
        lens = torch.randint(mean // 2, mean * 3 // 2 + 1, (P,), generator=gen)
        first = lens.cumsum(0) - lens
        S = int(lens.sum())
        t = (torch.arange(S) - first.repeat_interleave(lens)) / lens.repeat_interleave(lens)
        sdf = (0.3 - 0.6 * t + 0.05 * torch.randn(S, generator=gen)).float().to(dev)
        pi = _hip.mark_ordered(torch.stack([first, lens], 1).contiguous().to(dev), total=S)
        return dict(sdf=sdf, g=torch.randn(S, generator=gen).to(dev), pack_infos=pi)

    def calls(case, fused):
        """(forward, forward + backward, backward alone on a kept graph) of one route, inv_s a learnable GPU scalar"""
        x = case["sdf"].clone().requires_grad_(True)
        s = torch.tensor(INV_S, device=dev, requires_grad=True)
        pi, g = case["pack_infos"], case["g"]

        def forward():
            nu.FUSED_SDF_TO_ALPHA = fused
            return nu.neus_ray_sdf_to_alpha(x, s) if pi is None else nu.neus_packed_sdf_to_alpha(x, s, pi)

        def both():
            x.grad = s.grad = None
            forward().backward(g)

        kept = forward()

        def backward():
            x.grad = s.grad = None
            kept.backward(g, retain_graph=True)

        return forward, both, backward

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

    def alternated(fused, chain, iters):
        tf, tc = [], []
        for _ in range(args.rounds):
            tf.append(timed(fused, iters))
            tc.append(timed(chain, iters))
        f, c = statistics.median(tf), statistics.median(tc)
        return {"fused_ms": round(f, 4), "chain_ms": round(c, 4), "speedup": round(c / f, 3),
                "fused_rounds_ms": [round(t, 4) for t in tf], "chain_rounds_ms": [round(t, 4) for t in tc]}

    saved = nu.FUSED_SDF_TO_ALPHA
    try:
        if args.trace:
            case = pack_case(4096, 30)
            sigma = torch.rand(64, device=dev)
            phases = []
            for fused in (True, False):
                forward, _, backward = calls(case, fused)
                phases += [forward, backward]
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
        res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inv_s": INV_S, "rows": {}, "packs": {}}
        cases = [("rows", f"{R}x{n}", row_case(R, n)) for R, n in ROWS] + [("packs", f"{P}x~{m}", pack_case(P, m)) for P, m in PACKS]
        for group, name, case in cases:
            S = case["sdf"].numel()
            f_fwd, f_both, _ = calls(case, True)
            c_fwd, c_both, _ = calls(case, False)
            with torch.no_grad():
                a_f, a_c = f_fwd(), c_fwd()
            # a round of the faster route lasts about WINDOW_MS: calls of 0.014 ms timed 200 at a time measure the clock and the scheduler
            iters = {k: max(200, int(WINDOW_MS / timed(fn, 50))) for k, fn in (("forward", f_fwd), ("forward_backward", f_both))}
            r = {"samples": S, "iters": iters, "max_abs_alpha_difference": (a_f - a_c).abs().max().item(),
                 "forward": alternated(f_fwd, c_fwd, iters["forward"]),
                 "forward_backward": alternated(f_both, c_both, iters["forward_backward"])}
            res[group][name] = r
            print(group, name, "forward", r["forward"]["fused_ms"], r["forward"]["chain_ms"], "forward + backward",
                  r["forward_backward"]["fused_ms"], r["forward_backward"]["chain_ms"], flush=True)
        res["default_supported"] = all(r[k]["fused_ms"] <= r[k]["chain_ms"] for grp in ("rows", "packs") for r in res[grp].values()
                                       for k in ("forward", "forward_backward"))
        print("fused not slower in any row:", res["default_supported"], flush=True)
        merge_into(args.out, **res)
    finally:
        nu.FUSED_SDF_TO_ALPHA = saved


if __name__ == "__main__":
    main()
