#!/usr/bin/env python
"""tools/exp_neus_upsample.py -- the fused NeuS up-sampling stage measured on one GPU -> profiles/neus_upsample.json.

Workload: neus_ray_query_coarse_multi_upsample on an analytic sphere SDF (so that the stages, not a network, are what is timed),
4096 and 65 536 rays, num_coarse = 64, num_fine = 64, four stages, unperturbed, compression off, no rgb / normals.  The fused route
(FUSED_UPSAMPLE = True: one launch per stage) and the torch route (False: the reference's op chain with a full sort) run in
alternated rounds on the same inputs; a round is the mean of ITERS queries between two events after a warm-up, the figure is the
median of the rounds.  Also: the stage alone (kernel against op chain) at the first and the last stage's row lengths, the device
kernels per stage on each route as the torch profiler sees them, and the kernel's deviation from the float64 restatement
(tests/neus_coarse_ref.py) next to the float32 restatement's own (e_ref) on the parity cases of tests/test_neus_upsample_gpu.py.

    python tools/exp_neus_upsample.py [--rays 4096 65536] [--rounds 7] [--iters 200] [--out profiles/neus_upsample.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

QUERY = dict(compression=False, with_rgb=False, with_normal=False, num_coarse=64, num_fine=64, upsample_inv_s_factors=[1, 2, 4, 8])


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


def alternated(fused, plain, rounds, iters):
    tf, tp = [], []
    for _ in range(rounds):
        tf.append(timed(fused, iters))
        tp.append(timed(plain, iters))
    f, p = statistics.median(tf), statistics.median(tp)
    return {"fused_ms": round(f, 4), "torch_ms": round(p, 4), "speedup": round(p / f, 3),
            "fused_rounds_ms": [round(t, 4) for t in tf], "torch_rounds_ms": [round(t, 4) for t in tp]}


def device_kernels(fn):
    """names of the device kernels one call of fn launches, as the torch profiler records them"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def rays_on(dev, n_rays):
    import neus_coarse_ref as ref
    g = torch.Generator().manual_seed(0)
    d = torch.cat([0.12 * (torch.rand(n_rays, 2, generator=g) * 2 - 1), torch.ones(n_rays, 1)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    return dict(num_rays=n_rays, rays_o=torch.tensor(ref.ORIGIN).expand(n_rays, 3).contiguous().to(dev), rays_d=d.to(dev),
                near=torch.full((n_rays,), ref.NEAR, device=dev), far=torch.full((n_rays,), ref.FAR, device=dev),
                rays_inds=torch.arange(n_rays, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neus_upsample.json"))
    args = ap.parse_args()
    import neus_coarse_ref as ref
    from nr3d_lib_amd.bindings import _neus_upsample as U
    from nr3d_lib_amd.graphics.neus import neus_ray_query as rq
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    model = ref.SphereModel()
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "max_row": U.MAX_ROW,
           "query": {k: v for k, v in QUERY.items()}, "queries": {}, "stage_alone": {}, "kernels_per_stage": {}, "deviation": {}}

    def route(fused, fn):
        def run():
            rq.FUSED_UPSAMPLE = fused
            return fn()
        return run

    for n_rays in args.rays:
        rays = rays_on(dev, n_rays)
        query = lambda: rq.neus_ray_query_coarse_multi_upsample(model, rays, **QUERY)    # noqa: E731
        rq.FUSED_UPSAMPLE = True
        t_fused = query()[0]['t']
        rq.FUSED_UPSAMPLE = False
        t_plain = query()[0]['t']
        r = alternated(route(True, query), route(False, query), args.rounds, args.iters)
        r["max_abs_t_difference"] = (t_fused - t_plain).abs().max().item()
        res["queries"][str(n_rays)] = r
        print("query", n_rays, r["fused_ms"], r["torch_ms"], r["speedup"], flush=True)
        # the stage alone at the first (65 + 65) and the last (260 + 65) stage's row lengths
        for n in (65, 260):
            depth = torch.linspace(ref.NEAR, ref.FAR, n, device=dev).expand(n_rays, n).contiguous()
            sdf = (rays['rays_o'][:, None, :] + rays['rays_d'][:, None, :] * depth[..., None]).norm(dim=-1) - ref.RADIUS
            stage = lambda: rq._row_stage(depth, sdf, 65, 64.0, False, False)              # noqa: E731
            r = alternated(route(True, stage), route(False, stage), args.rounds, args.iters)
            res["stage_alone"][f"{n_rays}x({n}+65)"] = r
            print("stage", n_rays, n, r["fused_ms"], r["torch_ms"], r["speedup"], flush=True)
            if n_rays == args.rays[0] and n == 65:
                for name, fused in (("fused", True), ("torch", False)):
                    try:
                        names = device_kernels(route(fused, stage))
                        res["kernels_per_stage"][name] = {"count": len(names), "names": sorted({n[:96] for n in names})}
                    except Exception as e:                                                 # the profiler, not the measurement
                        res["kernels_per_stage"][name] = {"count": None, "error": repr(e)}
                print("kernels per stage", {k: v["count"] for k, v in res["kernels_per_stage"].items()}, flush=True)
    rq.FUSED_UPSAMPLE = True

    # the kernel's deviation from the float64 restatement on the parity cases, next to the float32 restatement's own
    fan = ref.fan_rays()
    for n, m in ((17, 9), (65, 65)):
        depth = torch.linspace(ref.NEAR, ref.FAR, n).expand(64, n).contiguous()
        sdf = ((fan['rays_o'][:, None, :] + fan['rays_d'][:, None, :] * depth[..., None]).norm(dim=-1) - ref.RADIUS).contiguous()
        u = ref.shared_u(m)
        for est in (False, True):
            for inv_s in (64, 128, 256, 512):
                fine = U.upsample_stage(depth.to(dev), sdf.to(dev), u.to(dev), float(inv_s), est)[0].cpu()
                r32, r64 = ref.stage(depth, sdf, u, float(inv_s), est, torch.float32), ref.stage(depth, sdf, u, float(inv_s), est, torch.float64)
                res["deviation"][f"n{n}_m{m}_est{int(est)}_inv_s{inv_s}"] = {
                    "kernel": (fine.double() - r64['fine']).abs().max().item(),
                    "e_ref": (r32['fine'].double() - r64['fine']).abs().max().item(),
                    "min_weight_sum": r64['wsum'].min().item()}
    worst = max(res["deviation"].values(), key=lambda v: v["kernel"] / max(v["e_ref"], 1e-30))
    print("deviation, worst kernel / e_ref:", worst, flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
