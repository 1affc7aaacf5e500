#!/usr/bin/env python
"""tools/exp_forest_ray_test.py -- ForestBlockSpace.ray_test measured on one GPU: the fused route (models.spatial.forest.
FUSED_FOREST_RAY_TEST: one octree descent per ray, csrc/forest_ray_test.hip) against the dense torch route (every ray against every
block box) -> profiles/forest_ray_test.json.

What is timed is a whole ``ray_test`` call with its host wait (both routes wait inside the call: the fused one for its two totals, the
dense one in its nonzero() calls), same process, same rays, near = 0.05 and a far beyond the forest.  The two routes alternate in rounds
of at least WINDOW_MS each (a round = the mean of as many calls as fill the window, between two host clock readings; the call's own
wait ends the work); the figure is the median of the rounds.  Rows:
  * "plus7": the 7-block forest of tools/exp_neus_forest_query.py, 4096 rays -- at least 7 rounds; the relative range of its rounds
    per route ((max - min) / median, the largest over its rows and routes) is the run's ``spread``;
  * "strip": a street-like strip of 29 blocks (level 5), 4096 rays;
  * "cube512": a full level-3 cube, 4096 and 65 536 rays;
  * "cube4096": a full level-4 cube, 4096 rays;
  each with rays from outside (a pinhole in front of the forest) and from inside (origins in occupied blocks, random directions);
  * "neus_query": the forest NeuS march-occ query of tools/exp_neus_forest_query.py (packs of 30) INCLUDING its ray test.
``fused_wins`` of a row: dense - fused > spread x the larger of the two.  ``default_on``: true in every row -- what
FUSED_FOREST_RAY_TEST's default has to follow; otherwise the rows sorted by rays x blocks give the threshold (``fit``).

    python tools/exp_forest_ray_test.py [--rounds 3] [--rounds-plus7 7] [--out profiles/forest_ray_test.json]

Launches per call, from the profiler and not from a count of the code (a run of its own, no counters):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o raytest -- python tools/exp_forest_ray_test.py --trace
    python tools/exp_forest_ray_test.py --read-trace DIR     # no GPU needed: splits DIR's kernel trace at the marker kernel
``--trace`` runs, on plus7 x 4096 rays from outside, TRACE_ITERS calls of each route with one launch of a marker kernel
(k_tau_to_alpha_fwd, which neither route uses) in front of each phase and behind the last."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "forest_ray_test.json")
WINDOW_MS = 250.0
TRACE_ITERS = 10
TRACE_PHASES = ("fused", "dense")
MARKER = "k_tau_to_alpha_fwd"
FIELDS = ("rays_inds", "seg_pack_infos", "seg_entries", "near", "far")
PLUS7 = [(1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)]
QUERY = dict(with_rgb=False, with_normal=False, coarse_step_cfg=None, num_fine=8, upsample_inv_s_factors=[1, 4, 16])
MARCH = dict(step_size=0.023, max_steps=256)


def merge_into(path, **sections):
    res = json.load(open(path)) if os.path.exists(path) else {}
    res.update(sections)
    os.makedirs(os.path.dirname(path), exist_ok=True)
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
    merge_into(out, launches=dict(source="rocprofv3 --kernel-trace --stats, a run of its own; plus7, 4096 rays from outside, near and far "
                                         "numbers, return_rays; kernels only (memory copies are not in a kernel trace)",
                                  iters=TRACE_ITERS, **launches))
    print({k: v["per_call"] for k, v in launches.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rounds-plus7", type=int, default=7)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--read-trace", default=None)
    args = ap.parse_args()
    if args.read_trace:
        return read_trace(args.read_trace, args.out)

    import numpy as np
    import torch
    from nr3d_lib_amd.bindings import _pack_ops
    from nr3d_lib_amd.models.spatial import ForestBlockSpace
    from nr3d_lib_amd.models.spatial import forest as F
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    assert args.rounds_plus7 >= 7, "the 7-block forest sets the spread: at least 7 rounds"
    dev = torch.device("cuda:0")

    def space_of(corners, level, origin, size):
        s = ForestBlockSpace(device=dev)
        s.populate(mode="from_corners", corners=corners, level=level, world_origin=origin, world_block_size=size)
        return s

    def cube(level):
        n = 1 << level
        return [(x, y, z) for x in range(n) for y in range(n) for z in range(n)]

    forests = {
        "plus7": space_of(PLUS7, 2, [-2., -2, -2], 1.0),
        "strip": space_of([(x, 3, 1) for x in range(32) if x not in (5, 6, 20)], 5, [-10., 0, 0], [12.5, 12.5, 6.25]),
        "cube512": space_of(cube(3), 3, [-4., -4, -4], 1.0),
        "cube4096": space_of(cube(4), 4, [-8., -8, -8], 1.0),
    }

    def rays(space, R, where):
        g = torch.Generator().manual_seed(R)
        box = space.get_aabb().cpu()
        centre, half = (box[0] + box[1]) / 2, (box[1] - box[0]) / 2
        if where == "outside":                                    # a pinhole in front of the forest's -x face, looking at it
            o = (centre - torch.tensor([1.0, 0, 0]) * (half[0] + 1.5 * half[1:].max())).repeat(R, 1)
            d = torch.cat([torch.ones(R, 1), 0.5 * (torch.rand(R, 2, generator=g) * 2 - 1)], -1)
        else:                                                     # inside occupied blocks, every direction
            k = space.block_ks.cpu()[torch.randint(0, space.n_trees, (R,), generator=g)].float()
            o = (k + torch.rand(R, 3, generator=g)) * space.world_block_size.cpu() + space.world_origin.cpu()
            d = torch.randn(R, 3, generator=g)
        d = d / d.norm(dim=-1, keepdim=True)
        return o.to(dev).contiguous(), d.to(dev).contiguous(), 0.05, float(4 * half.max())

    def call(space, r, fused):
        F.FUSED_FOREST_RAY_TEST = fused
        return space.ray_test(r[0], r[1], near=r[2], far=r[3])

    def timed(fn, iters):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def alternated(fused, dense, rounds):
        for fn in (fused, dense):                                 # every shape warm
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        iters = {k: max(2, int(1.2 * WINDOW_MS / timed(fn, 50)) + 1) for k, fn in (("fused", fused), ("dense", dense))}
        while True:                                               # a route whose shortest round falls below the window is taken again
            t = {"fused": [], "dense": []}
            for _ in range(rounds):
                t["fused"].append(timed(fused, iters["fused"]))
                t["dense"].append(timed(dense, iters["dense"]))
            short = [k for k in t if iters[k] * min(t[k]) < WINDOW_MS]
            if not short:
                break
            for k in short:
                iters[k] = int(iters[k] * 1.5) + 1
        f, c = statistics.median(t["fused"]), statistics.median(t["dense"])
        return {"fused_ms": round(f, 4), "dense_ms": round(c, 4), "speedup": round(c / f, 3), "iters": iters,
                "shortest_round_ms": round(min(iters[k] * min(t[k]) for k in t), 1),
                "range_over_median": {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in t.items()},
                "fused_rounds_ms": [round(x, 4) for x in t["fused"]], "dense_rounds_ms": [round(x, 4) for x in t["dense"]]}

    default = F.FUSED_FOREST_RAY_TEST
    try:
        if args.trace:
            r = rays(forests["plus7"], 4096, "outside")
            phases = [lambda f=f: call(forests["plus7"], r, f) for f in (True, False)]
            sigma = torch.rand(64, device=dev)
            for fn in phases:                                      # code objects loaded, allocator warm
                fn()
            torch.cuda.synchronize()
            for fn in phases:
                _pack_ops.tau_to_alpha_forward(sigma, sigma)
                for _ in range(TRACE_ITERS):
                    fn()
            _pack_ops.tau_to_alpha_forward(sigma, sigma)
            torch.cuda.synchronize()
            return

        res = {"device": torch.cuda.get_device_name(0), "window_ms": WINDOW_MS, "rounds": args.rounds, "rounds_plus7": args.rounds_plus7,
               "default_at_measurement": default, "rows": {}}
        plan = [("plus7", 4096), ("strip", 4096), ("cube512", 4096), ("cube512", 65536), ("cube4096", 4096)]
        for name, R in plan:
            space = forests[name]
            for where in ("outside", "inside"):
                r = rays(space, R, where)
                a, b = call(space, r, True), call(space, r, False)
                row = {"rays": R, "blocks": int(space.n_trees), "rays_x_blocks": R * int(space.n_trees), "hit_rays": int(a["num_rays"]),
                       "segments": int(a["seg_entries"].numel()),
                       "identical_but_tie_order": a["num_rays"] == b["num_rays"] and all(torch.equal(a[k], b[k]) for k in FIELDS)}
                del a, b
                row.update(alternated(lambda: call(space, r, True), lambda: call(space, r, False),
                                      args.rounds_plus7 if name == "plus7" else args.rounds))
                res["rows"][f"{name} {R} rays {where}"] = row
                print(name, R, where, row["segments"], "fused", row["fused_ms"], "dense", row["dense_ms"], row["identical_but_tie_order"],
                      flush=True)
                torch.cuda.empty_cache()

        # the forest NeuS march-occ query with its ray test in front
        import test_neus_forest_query_gpu as scene_of
        from nr3d_lib_amd.graphics.neus import neus_forest_ray_query as fq
        model = scene_of.scene(dev)[0]
        g = torch.Generator().manual_seed(0)
        d = torch.cat([torch.ones(4096, 1), 0.25 * (torch.rand(4096, 2, generator=g) * 2 - 1)], -1)
        d = (d / d.norm(dim=-1, keepdim=True)).to(dev)
        o = torch.tensor([-3.5, -0.5, -0.5]).repeat(4096, 1).to(dev)

        def query(fused):
            F.FUSED_FOREST_RAY_TEST = fused
            model.sdf_block_inds.clear()
            with torch.no_grad():
                rt = model.space.ray_test(o, d, near=0.05, far=8.0)
                return fq.neus_forest_ray_query_march_occ_multi_upsample(model, rt, march_cfg=MARCH, **QUERY)
        row = {"rays": 4096, "blocks": 7, "rays_x_blocks": 4096 * 7, "query": dict(QUERY), "march": MARCH}
        row.update(alternated(lambda: query(True), lambda: query(False), args.rounds_plus7))
        res["rows"]["neus_query plus7 4096 rays"] = row
        print("neus_query", "fused", row["fused_ms"], "dense", row["dense_ms"], flush=True)

        small = [r for k, r in res["rows"].items() if "plus7" in k]
        res["spread"] = max(max(r["range_over_median"].values()) for r in small)
        for r in res["rows"].values():
            r["fused_wins"] = bool(r["dense_ms"] - r["fused_ms"] > res["spread"] * max(r["dense_ms"], r["fused_ms"]))
        res["default_on"] = all(r["fused_wins"] for r in res["rows"].values())
        by_pairs = sorted(res["rows"].values(), key=lambda r: r["rays_x_blocks"])
        res["fit"] = [{"rays_x_blocks": r["rays_x_blocks"], "speedup": r["speedup"], "fused_wins": r["fused_wins"]} for r in by_pairs]
        print("spread", res["spread"], "fused wins every row:", res["default_on"], flush=True)
        merge_into(args.out, **res)
    finally:
        F.FUSED_FOREST_RAY_TEST = default


if __name__ == "__main__":
    main()
