#!/usr/bin/env python
"""tools/exp_neus_composite.py -- the fused NeuS render composite (neus_render.FUSED_NEUS_COMPOSITE) measured on one GPU
-> profiles/neus_composite.json.

The fused route (one launch each way, bindings._neus_composite) against the reference's op chain (the switch off: same library, same
process) on the same inputs, through ``composite_volume_buffer`` in training mode: 'batched' buffers of 4096 x 128 and 65 536 x 128
samples and of 262 144 x 1 (a sphere-traced buffer); 'packed' buffers of 4096 and 65 536 rays of about 30 and 300 samples (lengths
uniform in [len / 2, 3 len / 2], tiling the buffer and marked ordered, as a marcher's); each with rgb only and with rgb + normals.
Forward (no gradient recorded), and forward + backward from a loss on every rendered output.  A round is the mean of ITERS calls between
two events after a warm-up, ITERS (the same for both routes) chosen per case so that the fused route's round lasts about WINDOW_MS; the
two routes alternate, the figure is the median of the rounds.  ``default_supported``: the fused route is not slower in any row -- what
FUSED_NEUS_COMPOSITE's default has to follow.

    python tools/exp_neus_composite.py [--rounds 5] [--out profiles/neus_composite.json]
    python tools/exp_neus_composite.py --variant wave_per_row --lib LIB     # the rows cases on a library built with another lane mapping
                                                                            # (-DNR3D_NEUS_ROWS_MIN_LANES=64) -> "lane_mapping" in the JSON
    python tools/exp_neus_composite.py --yardstick LOG     # fold the "YARDSTICK ..." lines of a `pytest -s tests/test_neus_render_gpu.py` log into the JSON

Launches per route, from the profiler and not from a count of the code (a run of its own, no counters):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o composite -- python tools/exp_neus_composite.py --trace
    python tools/exp_neus_composite.py --read-trace DIR    # no GPU needed: splits DIR's kernel trace at the marker kernel, adds "launches"
``--trace`` runs, on 4096 x 128 rows and on 4096 packs of about 30 with rgb + normals, TRACE_ITERS calls of each phase (fused | chain) x
(forward | backward) with one launch of a marker kernel (k_tau_to_alpha_fwd, which neither route uses) in front of each phase and behind
the last."""
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
OUT = os.path.join(ROOT, "profiles", "neus_composite.json")
ROWS = ((4096, 128), (65536, 128), (262144, 1))
PACKS = ((4096, 30), (4096, 300), (65536, 30), (65536, 300))
TRACE_ITERS = 10
WINDOW_MS = 100.0
TRACE_PHASES = tuple(f"{lay} {route} {d}" for lay in ("rows", "packs") for route in ("fused", "chain") for d in ("forward", "backward"))
MARKER = "k_tau_to_alpha_fwd"
QUANTITIES = ("g_alpha", "g_t", "g_rgb", "g_nablas", "vw", "mask", "depth", "rgb", "normals")


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
        m = re.search(r"YARDSTICK (.*?): rel err ([0-9.e+-]+) .*ratio ([0-9.infa]+)", line)
        if m and m.group(3) not in ("inf", "nan"):
            what = next((k for k in QUANTITIES if m.group(1).endswith(k) or f" {k}" in m.group(1)), "other")
            by.setdefault(what, []).append((float(m.group(3)), m.group(1), float(m.group(2))))
    merge_into(out, yardstick_note="ratio = error / (torch fp32 chain's error), both relative to the tensor's maximum against the float64 "
                                   "evaluation; the bound is 4, and a ratio above it passes while the error is below 1e-5",
               yardstick={k: {"checks": len(v), "largest_ratio": max(v)[0], "at": max(v)[1], "rel_err_there": max(v)[2],
                              "largest_rel_err": max(e for _, _, e in v),
                              "median_ratio": round(statistics.median(r for r, _, _ in v), 3)} for k, v in sorted(by.items())})
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
    merge_into(out, launches=dict(source="rocprofv3 --kernel-trace --stats, a run of its own; 4096 x 128 rows and 4096 packs of about 30, rgb + "
                                         "normals, rays_inds_hit given; backward = the backward pass alone", iters=TRACE_ITERS, **launches))
    print({k: v["per_call"] for k, v in launches.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--read-trace", default=None)
    ap.add_argument("--yardstick", default=None)
    ap.add_argument("--lib", default=None, help="load this build of libnr3d_hip.so instead of the package's")
    ap.add_argument("--variant", default=None, help="rows cases only, stored under lane_mapping[VARIANT]")
    args = ap.parse_args()
    if args.read_trace:
        return read_trace(args.read_trace, args.out)
    if args.yardstick:
        return read_yardstick(args.yardstick, args.out)

    import torch
    from nr3d_lib_amd import _hip
    from nr3d_lib_amd.bindings import _pack_ops
    from nr3d_lib_amd.graphics.neus import neus_render as nr
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if args.lib:
        _hip.LIB_PATH = os.path.abspath(args.lib)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)

    def fields(shape, R):
        n = shape[-1] if len(shape) == 2 else 1
        return dict(opacity_alpha=(torch.rand(shape, generator=gen) ** 3).to(dev), t=torch.rand(shape, generator=gen).to(dev),
                    rgb=torch.rand(*shape, 3, generator=gen).to(dev), nablas=torch.randn(*shape, 3, generator=gen).to(dev),
                    rays_inds_hit=torch.randperm(R + R // 8, generator=gen)[:R].to(dev), num_rays=R + R // 8)

    def row_case(R, n):
        return dict(type="batched", **fields((R, n), R))

    def pack_case(P, mean):
        lens = torch.randint(mean // 2, mean * 3 // 2 + 1, (P,), generator=gen)
        first = lens.cumsum(0) - lens
        S = int(lens.sum())
        pi = _hip.mark_ordered(torch.stack([first, lens], 1).contiguous().to(dev), total=S)
        return dict(type="packed", pack_infos_hit=pi, **fields((S,), P))

    def calls(case, fused, normals):
        """(forward without a graph, forward + backward, backward alone on a kept graph) of one route"""
        leaves = {k: case[k].clone().requires_grad_(True) for k in ("opacity_alpha", "t", "rgb", "nablas")}
        num_rays = case["num_rays"]
        cot = {k: torch.randn(num_rays, *s, generator=gen).to(dev) for k, s in
               (("mask_volume", ()), ("depth_volume", ()), ("rgb_volume", (3,)), ("normals_volume", (3,)))}

        def render(grad):
            nr.FUSED_NEUS_COMPOSITE = fused
            buf = dict(case, **(leaves if grad else {k: v.detach() for k, v in leaves.items()}))
            return nr.composite_volume_buffer(buf, num_rays, with_rgb=True, with_normal=normals, training=True)

        def forward():
            with torch.no_grad():
                return render(False)

        def loss_of(out):
            return sum((v * cot[k]).sum() for k, v in out.items())

        def zero():
            for v in leaves.values():
                v.grad = None

        def both():
            zero()
            loss_of(render(True)).backward()

        kept = loss_of(render(True))

        def backward():
            zero()
            kept.backward(retain_graph=True)

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

    saved = nr.FUSED_NEUS_COMPOSITE
    try:
        if args.trace:
            sigma = torch.rand(64, device=dev)
            phases = []
            for case in (row_case(4096, 128), pack_case(4096, 30)):
                for fused in (True, False):
                    forward, _, backward = calls(case, fused, True)
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
        res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": WINDOW_MS, "rows": {}, "packs": {}}
        cases = [("rows", f"{R}x{n}", (row_case, R, n)) for R, n in ROWS] + [("packs", f"{P}x~{m}", (pack_case, P, m)) for P, m in PACKS]
        if args.variant:
            cases = [c for c in cases if c[0] == "rows"]
        for group, name, (make, a, b) in cases:
            case = make(a, b)
            for normals in (False, True):
                f_fwd, f_both, _ = calls(case, True, normals)
                c_fwd, c_both, _ = calls(case, False, normals)
                o_f, o_c = f_fwd(), c_fwd()
                diff = max(((o_f[k] - o_c[k]).abs().max() / o_c[k].abs().max()).item() for k in o_f)
                iters = {k: max(20, int(WINDOW_MS / timed(fn, 10))) for k, fn in (("forward", f_fwd), ("forward_backward", f_both))}
                r = {"samples": case["opacity_alpha"].numel(), "iters": iters, "max_rel_output_difference": diff,
                     "forward": alternated(f_fwd, c_fwd, iters["forward"]),
                     "forward_backward": alternated(f_both, c_both, iters["forward_backward"])}
                key = f"{name} {'rgb+normals' if normals else 'rgb'}"
                res[group][key] = r
                print(group, key, "forward", r["forward"]["fused_ms"], r["forward"]["chain_ms"], "forward + backward",
                      r["forward_backward"]["fused_ms"], r["forward_backward"]["chain_ms"], flush=True)
                del f_fwd, f_both, c_fwd, c_both, o_f, o_c
            del case
            torch.cuda.empty_cache()
        if args.variant:
            old = json.load(open(args.out)).get("lane_mapping", {}) if os.path.exists(args.out) else {}
            old[args.variant] = {k: {d: {"fused_ms": r[d]["fused_ms"], "fused_rounds_ms": r[d]["fused_rounds_ms"]}
                                     for d in ("forward", "forward_backward")} for k, r in res["rows"].items()}
            return merge_into(args.out, lane_mapping=old)
        res["default_supported"] = all(r[k]["fused_ms"] <= r[k]["chain_ms"] for grp in ("rows", "packs") for r in res[grp].values()
                                       for k in ("forward", "forward_backward"))
        res["rows_lost"] = [f"{grp} {name} {k}" for grp in ("rows", "packs") for name, r in res[grp].items()
                            for k in ("forward", "forward_backward") if r[k]["fused_ms"] > r[k]["chain_ms"]]
        print("fused not slower in any row:", res["default_supported"], res["rows_lost"], flush=True)
        merge_into(args.out, **res)
    finally:
        nr.FUSED_NEUS_COMPOSITE = saved


if __name__ == "__main__":
    main()
