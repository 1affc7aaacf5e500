#!/usr/bin/env python
"""tools/exp_importance.py -- pixel importance sampling (models/importance.py: FUSED_IMPORTANCE) measured on one GPU -> profiles/importance.json.

The fused route (csrc/importance.hip) against the reference's op chain (the switch off: same process, same maps) on maps of
7 x 128 x 128 (the reference's own timing case) and 1000 x 64 x 64, filled uniform(0.2, 1) and updated once:
    ErrorMap.sample_img_pixel at 4096, 16 384 and 65 536 samples; ImpSampler.sample_img_pixel (16 384) with one and with three maps;
    update_error_map (16 384 samples) with a scalar frame and with per-sample frames, each with the reference's `val < 0` check (a host
    wait) and without it; construct_cdf.
A round is the mean of ITERS calls between two events after a warm-up, ITERS (the same for both routes) chosen per row so that the
faster route's round lasts at least a quarter of a second; the routes alternate; the figure is the median of the rounds.  ``wins``: the
fused route's SLOWEST round is below the chain's FASTEST round.  ``calls_that_win``: the calls that win in every row -- what
models.importance.FUSED_CALLS has to follow.

    python tools/exp_importance.py [--rounds 7] [--out profiles/importance.json]

Launches per call, from the profiler and not from a count of the code (a run of its own, no counters):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o importance -- python tools/exp_importance.py --trace
    python tools/exp_importance.py --read-trace DIR    # no GPU needed: splits DIR's kernel trace at the marker kernel, adds "launches"
``--trace`` runs TRACE_ITERS calls of each phase with one launch of a marker kernel (k_tau_to_alpha_fwd, which neither route uses) in
front of each phase and behind the last."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "importance.json")
SHAPES = ((7, 128, 128), (1000, 64, 64))
SAMPLE_SIZES = (4096, 16384, 65536)
N = 16384
TRACE_ITERS = 10
WINDOW_MS = 250.0
MARKER = "k_tau_to_alpha_fwd"
TRACE_CALLS = ("ErrorMap.sample_img_pixel", "ImpSampler.sample_img_pixel 3 maps", "update_error_map frames no check", "construct_cdf")
TRACE_PHASES = tuple(f"{route} {c}" for route in ("fused", "chain") for c in TRACE_CALLS)
KIND = {"ErrorMap.sample_img_pixel": "sample", "ImpSampler.sample_img_pixel": "sample", "update_error_map": "update",
        "construct_cdf": "construct_cdf"}


def merge_into(path, **sections):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res.update(sections)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def read_trace(trace_dir, out):
    f = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    cuts = [i for i, r in enumerate(rows) if MARKER in r["Kernel_Name"]]
    assert len(cuts) == len(TRACE_PHASES) + 1, f"{len(cuts)} marker launches in {f}"
    launches = {}
    for phase, a, b in zip(TRACE_PHASES, cuts[:-1], cuts[1:]):
        per = {}
        for r in rows[a + 1:b]:
            per[r["Kernel_Name"][:100]] = per.get(r["Kernel_Name"][:100], 0) + 1
        launches[phase] = {"per_call": (b - a - 1) / TRACE_ITERS, "kernels": {k: v / TRACE_ITERS for k, v in sorted(per.items())}}
    merge_into(out, launches=dict(source="rocprofv3 --kernel-trace --stats, a run of its own; 7 x 128 x 128, 16 384 samples",
                                  iters=TRACE_ITERS, **launches))
    print({k: v["per_call"] for k, v in launches.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--read-trace", default=None)
    args = ap.parse_args()
    if args.read_trace:
        return read_trace(args.read_trace, args.out)
    assert args.rounds >= 7, "the protocol wants at least 7 rounds"

    import torch
    from nr3d_lib_amd.bindings import _pack_ops
    from nr3d_lib_amd.models import importance as I
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)

    def make_map(shape):
        m = I.ErrorMap(shape[0], shape[1:], device=dev)
        m.error_map.copy_(torch.empty(shape).uniform_(0.2, 1, generator=gen))
        m.update_error_map(0, torch.rand([130, 2], generator=gen).to(dev), torch.rand([130], generator=gen).to(dev))
        m.construct_cdf()
        return m

    def cases(shape):
        """{row name: (callable, CHECK_VAL during it)}"""
        m = make_map(shape)
        one = I.ImpSampler({"a": (m, 0.5)})
        three = I.ImpSampler({"a": (m, 0.5), "b": (make_map(shape), 0.3), "c": (make_map(shape), 0.2)})
        xy, val = torch.rand([N, 2], generator=gen).to(dev), torch.rand([N], generator=gen).to(dev)
        frames = torch.randint(shape[0], [N], generator=gen).to(dev)
        out = {f"ErrorMap.sample_img_pixel {n}": (lambda n=n: m.sample_img_pixel(n), True) for n in SAMPLE_SIZES}
        out["ImpSampler.sample_img_pixel 1 map"] = (lambda: one.sample_img_pixel(N), True)
        out["ImpSampler.sample_img_pixel 3 maps"] = (lambda: three.sample_img_pixel(N), True)
        for check in (True, False):
            tag = "check" if check else "no check"
            out[f"update_error_map scalar {tag}"] = (lambda: m.update_error_map(3, xy, val), check)
            out[f"update_error_map frames {tag}"] = (lambda: m.update_error_map(frames, xy, val), check)
        out["construct_cdf"] = (m.construct_cdf, True)
        return out

    def route(fn, fused, check):
        def call():
            I.FUSED_IMPORTANCE, I.CHECK_VAL = fused, check
            return fn()
        return call

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

    saved = I.FUSED_IMPORTANCE, I.CHECK_VAL, I.FUSED_CALLS
    I.FUSED_CALLS = frozenset({"sample", "update", "construct_cdf"})      # the switch alone decides here
    try:
        if args.trace:
            c = cases(SHAPES[0])
            phases = [route(c[name if name != "ErrorMap.sample_img_pixel" else f"{name} {N}"][0], fused, False)
                      for fused in (True, False) for name in TRACE_CALLS]
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
        res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": WINDOW_MS, "rows": {}}
        for shape in SHAPES:
            tag = "x".join(map(str, shape))
            res["rows"][tag] = {}
            for name, (fn, check) in cases(shape).items():
                fused, chain = route(fn, True, check), route(fn, False, check)
                iters = max(50, int(WINDOW_MS / min(timed(fused, 20), timed(chain, 20))) + 1)
                tf, tc = [], []
                for _ in range(args.rounds):
                    tf.append(timed(fused, iters))
                    tc.append(timed(chain, iters))
                f, c = statistics.median(tf), statistics.median(tc)
                r = {"iters": iters, "fused_ms": round(f, 4), "chain_ms": round(c, 4), "speedup": round(c / f, 3),
                     "wins": max(tf) < min(tc), "fused_rounds_ms": [round(t, 4) for t in tf], "chain_rounds_ms": [round(t, 4) for t in tc]}
                res["rows"][tag][name] = r
                print(tag, name, r["fused_ms"], r["chain_ms"], r["speedup"], "wins" if r["wins"] else "LOSES", flush=True)
        kinds = {}
        for rows in res["rows"].values():
            for name, r in rows.items():
                k = next(v for p, v in KIND.items() if name.startswith(p))
                kinds[k] = kinds.get(k, True) and r["wins"]
        res["calls_that_win"] = sorted(k for k, v in kinds.items() if v)
        print("calls whose fused route wins in every row:", res["calls_that_win"], flush=True)
        merge_into(args.out, **res)
    finally:
        I.FUSED_IMPORTANCE, I.CHECK_VAL, I.FUSED_CALLS = saved


if __name__ == "__main__":
    main()
