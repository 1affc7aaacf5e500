#!/usr/bin/env python
"""tools/exp_nerfpp_march.py -- the fused NeRF++ shell marcher (nerfpp_raymarch.FUSED_NERFPP_MARCH) measured on one GPU ->
profiles/nerfpp_march.json.

The fused route (count, scan with the one readback, emit: bindings._nerfpp_march) against the reference's op chain (the switch off: same
library, same process) on the same rays: 4096 and 65 536 rays x max_steps 32, 64 and 256; 'box' + 'inverse_proportional' and
'spherical' + 'logarithm'; rays from inside the innermost shell (every shell valid) and the same rays with t_min between the two middle
shells (about half cut); with and without perturb.  radius_scale 1 .. 100, include_inf_distance on.  A round is the mean of ITERS calls
between two events after a warm-up, ITERS (the same for both routes) chosen per row so that the SLOWER route's round lasts about
WINDOW_MS; the two routes alternate, the figure is the median of the rounds.  Both routes wait for the device inside every call (the
fused route reads its totals back, the chain calls nonzero()), so a call is a whole march.  ``default_supported``: the fused route is
not slower in any row -- what FUSED_NERFPP_MARCH's default has to follow.  ``max_difference``: the largest difference between the two
routes' outputs over all rows without perturb (samples absolute, depths and deltas relative), and whether every integer output was equal.

    python tools/exp_nerfpp_march.py [--rounds 7] [--out profiles/nerfpp_march.json]
    python tools/exp_nerfpp_march.py --yardstick LOG   # fold the "YARDSTICK ..." lines of a `pytest -s tests/test_nerfpp_march_gpu.py
                                                       # tests/test_nerf_distant_query_gpu.py` log into the JSON

Launches per march, from the profiler and not from a count of the code (a run of its own, no counters):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o march -- python tools/exp_nerfpp_march.py --trace
    python tools/exp_nerfpp_march.py --read-trace DIR  # no GPU needed: splits DIR's kernel trace at the marker kernel, adds "launches"
``--trace`` runs, on 4096 rays x 64 steps ('box', 'inverse_proportional', inside), TRACE_ITERS calls of each of the four phases
(fused | chain) x (perturb off | on) with one launch of a marker kernel (k_tau_to_alpha_fwd, which neither route uses) in front of each
phase and behind the last."""
import argparse
import csv
import glob
import importlib
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "nerfpp_march.json")
RAYS = (4096, 65536)
STEPS = (32, 64, 256)
CONFIGS = (("box", "inverse_proportional"), ("spherical", "logarithm"))
AABB = [[-1.0, -2.0, -0.5], [1.0, 2.0, 0.5]]
MARCH = dict(radius_scale_min=1.0, radius_scale_max=100.0, include_inf_distance=True)
TRACE_ITERS = 10
WINDOW_MS = 250.0
TRACE_PHASES = ("fused", "fused perturb", "chain", "chain perturb")
MARKER = "k_tau_to_alpha_fwd"
QUANTITIES = ("depth_samples", "samples", "deltas to the far shell", "deltas", "opacity_alpha", "sigma", "rgb", " t")


def merge_into(path, **sections):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res.update(sections)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def read_yardstick(log, out):
    """the ratios the GPU tests printed: the count, the largest and the median per quantity, and the largest error"""
    by = {}
    for line in open(log):
        m = re.search(r"YARDSTICK (.*?): rel err ([0-9.e+-]+) torch fp32 ([0-9.e+-]+) ratio ([0-9.infa]+)", line)
        if m:
            what = next((k.strip() for k in QUANTITIES if m.group(1).endswith(k)), "other")
            ratio = float(m.group(4)) if m.group(4) not in ("inf", "nan") else None
            by.setdefault(what, []).append((ratio, float(m.group(2)), m.group(1)))
    merge_into(out, yardstick_note="ratio = error / (the torch chain's float32 error on the same inputs and device), both against the float64 "
                                   "evaluation and relative to the tensor's maximum (deltas to the far shell: element by element); the bound "
                                   "is 4, and a ratio above it passes while the error is below 1e-5; checks where the chain's error is "
                                   "exactly 0 have no ratio and count under no_ratio",
               yardstick={k: summary(v) for k, v in sorted(by.items())})
    print({k: len(v) for k, v in by.items()})


def summary(checks):
    rated = sorted(c for c in checks if c[0] is not None)
    out = {"checks": len(checks), "no_ratio": len(checks) - len(rated), "largest_error": max(e for _, e, _ in checks)}
    if rated:
        out.update(largest_ratio=rated[-1][0], error_there=rated[-1][1], at=rated[-1][2],
                   median_ratio=round(statistics.median(r for r, _, _ in rated), 3))
    return out


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
    merge_into(out, launches=dict(source="rocprofv3 --kernel-trace --stats, a run of its own; 4096 rays x 64 steps, box, "
                                         "inverse_proportional, every shell valid; kernels only (memory copies are not in a kernel trace)",
                                  iters=TRACE_ITERS, **launches))
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
    from nr3d_lib_amd.bindings import _pack_ops
    from nr3d_lib_amd.models.spatial import AABBSpace
    mod = importlib.import_module("nr3d_lib_amd.graphics.raymarch.nerfpp_raymarch")
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    space = AABBSpace(aabb=AABB, device=dev)

    def inside_rays(R):
        aabb = torch.tensor(AABB)
        c, h = (aabb[1] + aabb[0]) / 2, (aabb[1] - aabb[0]) / 2
        o = c + 0.4 * (torch.rand(R, 3, generator=gen) * 2 - 1) * h
        d = torch.randn(R, 3, generator=gen) * (0.5 + 2.0 * torch.rand(R, 1, generator=gen))
        return o.to(dev).contiguous(), d.to(dev).contiguous()

    def march(o, d, t_min, mode, interval, steps, perturb, fused):
        return mod.nerfpp_raymarch(space, o, d, t_min, None, perturb=perturb, max_steps=steps, sample_mode=mode, interval_type=interval,
                                   fused=fused, **MARCH)

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

    if args.trace:
        o, d = inside_rays(4096)
        t_min = torch.zeros(4096, device=dev)
        sigma = torch.rand(64, device=dev)
        phases = [lambda f=fused, p=perturb: march(o, d, t_min, "box", "inverse_proportional", 64, p, f)
                  for fused in (True, False) for perturb in (False, True)]
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

    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": WINDOW_MS, "march": MARCH, "rows": {}}
    diff = {"samples_abs": 0.0, "depth_samples_rel": 0.0, "deltas_rel": 0.0, "integers_equal": True}
    for R in RAYS:
        o, d = inside_rays(R)
        zero = torch.zeros(R, device=dev)
        for mode, interval in CONFIGS:
            for steps in STEPS:
                full = march(o, d, zero, mode, interval, steps, False, False)
                n = full.depth_samples.numel() // R
                assert full.depth_samples.numel() == R * n, "rays from inside: every shell valid"
                t = full.depth_samples.view(R, n)
                half = ((t[:, n // 2 - 1] + t[:, n // 2]) / 2).contiguous()
                del full, t
                for cut, t_min in (("all valid", zero), ("half cut", half)):
                    for perturb in (False, True):
                        name = f"{R}x{steps} {mode} {interval} {cut}{' perturb' if perturb else ''}"
                        f_fn = lambda: march(o, d, t_min, mode, interval, steps, perturb, True)       # noqa: E731
                        c_fn = lambda: march(o, d, t_min, mode, interval, steps, perturb, False)      # noqa: E731
                        a, b = f_fn(), c_fn()
                        row = {"shells": n, "samples": int(a.ridx.numel())}
                        if not perturb:
                            eq = all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("ridx_hit", "ridx", "pack_infos"))
                            diff["integers_equal"] = diff["integers_equal"] and eq
                            if eq:
                                rel = lambda x, y: float(((x - y).abs() / y.abs().clamp_min(1e-30)).max())   # noqa: E731
                                diff["samples_abs"] = max(diff["samples_abs"], float((a.samples - b.samples).abs().max()))
                                diff["depth_samples_rel"] = max(diff["depth_samples_rel"], rel(a.depth_samples, b.depth_samples))
                                diff["deltas_rel"] = max(diff["deltas_rel"], rel(a.deltas, b.deltas))
                        del a, b
                        iters = max(3, int(WINDOW_MS / max(timed(f_fn, 3), timed(c_fn, 3))))
                        row.update(iters=iters, **alternated(f_fn, c_fn, iters))
                        res["rows"][name] = row
                        print(name, row["samples"], "fused", row["fused_ms"], "chain", row["chain_ms"], flush=True)
    res["max_difference"] = diff
    res["default_supported"] = all(r["fused_ms"] <= r["chain_ms"] for r in res["rows"].values())
    print("fused not slower in any row:", res["default_supported"], diff, flush=True)
    merge_into(args.out, **res)


if __name__ == "__main__":
    main()
