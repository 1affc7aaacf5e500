#!/usr/bin/env python
"""tools/exp_dynamic_march.py -- the time-sliced occupancy march (occgrid_raymarch.FUSED_DYNAMIC_MARCH) measured on one GPU ->
profiles/dynamic_march.json.

What is timed is the accelerator's whole ``ray_march`` call including its host wait (both routes wait for the device inside the call:
the fused route reads its totals back, the chain reads the marcher's total and calls nonzero()), the fused route (lookup, static |
dynamic probe and per-sample gathers inside two launches: bindings._occ_grid.dynamic_ray_marching) against the chain (the reference's
sequence: lookup ops -> materialised [T, 128^3] union -> batched march -> gathers), same library, same process, same rays.

Rows: 4096 and 65 536 rays; T = 16 and T = 128 keyframes at 128^3 on a shell-like occupancy whose radius moves with the frame;
``OccGridAccelDynamic`` (dynamic only) and ``OccGridAccelStaticAndDynamic`` (a static shell OR-ed on).  step 2 sqrt(3) / 512, at most
512 samples per ray.  Every shape is warmed; a round is the mean of ITERS calls between two host clock readings around work that ends in
the call's own device wait (plus one synchronise), ITERS (the same for both routes) chosen per row so that the FASTER route's round
lasts at least WINDOW_MS; the two routes alternate, the figure is the median of the rounds.  ``default_supported``: the fused route is at
or below the chain in every row -- what FUSED_DYNAMIC_MARCH's default has to follow.  ``max_difference``: the largest difference between
the two routes' outputs per row (expected: none).

    python tools/exp_dynamic_march.py [--rounds 7] [--out profiles/dynamic_march.json]

Launches per march, from the profiler and not from a count of the code (a run of its own, no counters):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o march -- python tools/exp_dynamic_march.py --trace
    python tools/exp_dynamic_march.py --read-trace DIR   # no GPU needed: splits DIR's kernel trace at the marker kernel, adds "launches"
``--trace`` runs, on 4096 rays x T = 16, TRACE_ITERS calls of each of the four phases (fused | chain) x (dynamic | static + dynamic) with
one launch of a marker kernel (k_tau_to_alpha_fwd, which neither route uses) in front of each phase and behind the last."""
import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "dynamic_march.json")
RAYS = (4096, 65536)
FRAMES = (16, 128)
RES = 128
MARCH = dict(step_size=2 * 3 ** 0.5 / 512, max_steps=512)
TRACE_ITERS = 10
WINDOW_MS = 250.0
TRACE_PHASES = ("fused dynamic", "fused static+dynamic", "chain dynamic", "chain static+dynamic")
MARKER = "k_tau_to_alpha_fwd"
FIELDS = ("ridx_hit", "samples", "depth_samples", "deltas", "ridx", "pack_infos", "ts", "gidx")


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
        names = [r["Kernel_Name"] for r in rows[a + 1:b]]
        per = {}
        for n in names:
            per[n[:100]] = per.get(n[:100], 0) + 1
        launches[phase] = {"per_call": len(names) / TRACE_ITERS, "kernels": {k: v / TRACE_ITERS for k, v in sorted(per.items())}}
    merge_into(out, launches=dict(source="rocprofv3 --kernel-trace --stats, a run of its own; 4096 rays, T = 16, 128^3; kernels only "
                                         "(memory copies are not in a kernel trace)", iters=TRACE_ITERS, **launches))
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

    import numpy as np
    import torch
    from nr3d_lib_amd.bindings import _pack_ops
    from nr3d_lib_amd.models.accelerations.occgrid_accel import OccGridAccelDynamic, OccGridAccelStaticAndDynamic
    from nr3d_lib_amd.models.spatial import AABBDynamicSpace
    mod = importlib.import_module("nr3d_lib_amd.graphics.raymarch.occgrid_raymarch")
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    space = AABBDynamicSpace(device=dev)
    c = (torch.arange(RES, device=dev) + 0.5) / RES * 2 - 1
    radius = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).norm(dim=-1)

    def accel(T, static):
        """a shell of thickness 0.15 whose radius grows from 0.35 to 0.75 over the frames; the static part: a shell at 0.9"""
        keys = torch.linspace(-1, 1, T, device=dev)
        cfg = dict(resolution=RES, device=dev, init_cfg=dict(mode="constant", constant_value=0.0))
        if static:
            acc = OccGridAccelStaticAndDynamic(space, keys, occ_static_cfg={}, occ_dynamic_cfg={}, **cfg)
            acc.occ_static.occ_grid.copy_((radius > 0.88) & (radius < 0.95))
            stack = acc.occ_dynamic.occ_grid
        else:
            acc = OccGridAccelDynamic(space, keys, **cfg)
            stack = acc.occ.occ_grid
        for k in range(T):
            r0 = 0.35 + 0.4 * k / max(T - 1, 1)
            stack[k] = (radius > r0) & (radius < r0 + 0.15)
        return acc.eval()

    def rays(R):
        rng = np.random.default_rng(R)
        o = rng.standard_normal((R, 3))
        o = 4.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
        d = rng.uniform(-0.8, 0.8, (R, 3)) - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)     # noqa: E731
        tested = space.ray_test(f(o), f(d), normalized=True, rays_ts=f(rng.uniform(-1.1, 1.1, R)))
        return tested["rays_o"].contiguous(), tested["rays_d"].contiguous(), tested["rays_ts"].contiguous(), tested["near"], tested["far"]

    def march(acc, r, fused):
        mod.FUSED_DYNAMIC_MARCH = fused
        return acc.ray_march(r[0], r[1], r[2], r[3], r[4], **MARCH)

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def alternated(fused, chain, iters):
        tf, tc = [], []
        for _ in range(args.rounds):
            tf.append(timed(fused, iters))
            tc.append(timed(chain, iters))
        f, c = statistics.median(tf), statistics.median(tc)
        return {"fused_ms": round(f, 4), "chain_ms": round(c, 4), "speedup": round(c / f, 3),
                "fused_rounds_ms": [round(t, 4) for t in tf], "chain_rounds_ms": [round(t, 4) for t in tc]}

    default = mod.FUSED_DYNAMIC_MARCH
    try:
        if args.trace:
            r = rays(4096)
            accs = [accel(16, False), accel(16, True)]
            phases = [lambda a=a, f=f: march(a, r, f) for f in (True, False) for a in accs]
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

        res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": WINDOW_MS, "resolution": RES,
               "march": MARCH, "default_at_measurement": default, "rows": {}}
        for T in FRAMES:
            for static in (False, True):
                acc = accel(T, static)
                for R in RAYS:
                    r = rays(R)
                    name = f"{R} rays T={T} {'static+dynamic' if static else 'dynamic'}"
                    f_fn = lambda: march(acc, r, True)         # noqa: E731
                    c_fn = lambda: march(acc, r, False)        # noqa: E731
                    a, b = f_fn(), c_fn()
                    row = {"tested_rays": int(r[0].shape[0]), "hit_rays": int(a.num_hit_rays), "samples": int(a.ridx.numel())}
                    row["max_difference"] = {k: (float((getattr(a, k).double() - getattr(b, k).double()).abs().max())
                                                 if getattr(a, k).shape == getattr(b, k).shape else "shapes differ") for k in FIELDS}
                    row["identical"] = all(torch.equal(getattr(a, k), getattr(b, k)) for k in FIELDS)
                    del a, b
                    # the FASTER route's round lasts the window: estimated on 50 warm calls, with a fifth to spare; a row whose
                    # shortest round still falls below the window is taken again with twice the calls
                    iters = max(3, int(1.2 * WINDOW_MS / min(timed(f_fn, 50), timed(c_fn, 50))) + 1)
                    while True:
                        t = alternated(f_fn, c_fn, iters)
                        shortest = iters * min(t["fused_rounds_ms"] + t["chain_rounds_ms"])
                        if shortest >= WINDOW_MS:
                            break
                        iters *= 2
                    row.update(iters=iters, shortest_round_ms=round(shortest, 1), **t)
                    res["rows"][name] = row
                    print(name, row["samples"], "fused", row["fused_ms"], "chain", row["chain_ms"], "identical", row["identical"], flush=True)
                del acc
                torch.cuda.empty_cache()
        res["default_supported"] = all(r["fused_ms"] <= r["chain_ms"] for r in res["rows"].values())
        res["all_identical"] = all(r["identical"] for r in res["rows"].values())
        print("fused at or below the chain in every row:", res["default_supported"], "outputs identical:", res["all_identical"], flush=True)
        merge_into(args.out, **res)
    finally:
        mod.FUSED_DYNAMIC_MARCH = default


if __name__ == "__main__":
    main()
