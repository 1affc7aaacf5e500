#!/usr/bin/env python
"""tools/exp_neus_forest_query.py -- the forest NeuS march-occ query and its block-carrying up-sampling stage measured on one GPU
-> profiles/neus_forest_query.json.

Workload: neus_forest_ray_query_march_occ_multi_upsample on the 7-block "plus" forest of tests/test_neus_forest_query_gpu.py (an
analytic sphere SDF, so that the stages, not a network, are what is timed; per-block occupancy grids learnt from the sphere's
shell), 4096 and 65 536 rays from a pinhole towards the hub, num_fine = 8, factors [1, 4, 16], unperturbed, no rgb / normals, with
two march step sizes: packs of about 30 and of about 300 samples.  The fused route (FUSED_UPSAMPLE_FOREST = True: one launch per
factor) and the pack-op chain (False) run in alternated rounds on the same inputs; a round is the mean of ITERS queries between two
events after a warm-up, the figure is the median of the rounds.  Also the labelled stage alone against the unlabelled one on the
same marched samples, timed twice: "kernel" = the one C entry with and without labels on preallocated outputs (the launch and the kernel: the labelled
stage moves 8 B more per sample each way), "binding" = upsample_stage_packed_blocks against upsample_stage_packed as the drivers
call them (with the argument checks and 7 against 5 output allocations per call); and the largest |fused - chain| of the query's
depths.

FUSED_UPSAMPLE_FOREST defaults to True only if "fused" is below "chain" in every row of "queries".

    python tools/exp_neus_forest_query.py [--rays 4096 65536] [--rounds 7] [--iters 20] [--stage-iters 200] [--out profiles/...json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

QUERY = dict(with_rgb=False, with_normal=False, coarse_step_cfg=None, num_fine=8, upsample_inv_s_factors=[1, 4, 16])
MARCH = {"packs_of_30": dict(step_size=0.023, max_steps=256), "packs_of_300": dict(step_size=0.0023, max_steps=2048)}
SEG_KEYS = ('seg_block_inds', 'seg_entries', 'seg_exits', 'seg_pack_infos')


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


def alternated(fns, rounds, iters):
    """{name: fn} timed in alternated rounds -> {name: {ms: median, rounds_ms}}"""
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, iters))
    return {k: {"ms": round(statistics.median(v), 4), "rounds_ms": [round(x, 4) for x in v]} for k, v in t.items()}


def rays_towards_hub(model, dev, n_rays):
    g = torch.Generator().manual_seed(0)
    d = torch.cat([torch.ones(n_rays, 1), 0.25 * (torch.rand(n_rays, 2, generator=g) * 2 - 1)], -1)
    d = (d / d.norm(dim=-1, keepdim=True)).to(dev)
    o = torch.tensor([-3.5, -0.5, -0.5]).repeat(n_rays, 1).to(dev)
    return model.space.ray_test(o, d, near=0.05, far=8.0)


def stage_kernels(depth, sdf, bl, pi, u):
    """the C entry with and without labels, merge and need_sdf on, on outputs allocated once -> (labelled, unlabelled) callables"""
    from nr3d_lib_amd import _hip as H
    N, P, m, dev = depth.shape[0], pi.shape[0], u.shape[0], depth.device
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)       # noqa: E731
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)         # noqa: E731
    ws, fine, merged, sdf_m = f32(max(N, 1)), f32(P, m), f32(N + P * m), f32(N + P * m)
    bl_fine, bl_m, pidx, pi_out = i64(P, m), i64(N + P * m), i64(P, m), i64(P, 2)
    lib, st, p = H.lib(), H.stream_of(depth), H.ptr

    def labelled():
        H.check(lib.nr3d_neus_upsample_stage_packed(P, N, m, p(depth), p(sdf), p(bl), p(pi), p(u), 0, 64.0, 0, 1, 1, p(ws), p(fine),
                                                    p(bl_fine), p(merged), p(sdf_m), p(bl_m), p(pidx), p(pi_out), st))

    def unlabelled():
        H.check(lib.nr3d_neus_upsample_stage_packed(P, N, m, p(depth), p(sdf), None, p(pi), p(u), 0, 64.0, 0, 1, 1, p(ws), p(fine), None,
                                                    p(merged), p(sdf_m), None, p(pidx), p(pi_out), st))
    return labelled, unlabelled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--stage-iters", type=int, default=200, help="calls per round when one stage alone is timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neus_forest_query.json"))
    args = ap.parse_args()
    import test_neus_forest_query_gpu as scene_of
    from nr3d_lib_amd.bindings import _neus_upsample as U
    from nr3d_lib_amd.graphics.neus import neus_forest_ray_query as fq
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    model = scene_of.scene(dev)[0]
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "stage_iters": args.stage_iters,
           "lds_row": U.PACKED_LDS_ROW, "query": dict(QUERY), "march": MARCH, "queries": {}, "stage_alone": {}}

    def route(fused, fn):
        def run():
            fq.FUSED_UPSAMPLE_FOREST = fused
            return fn()
        return run

    default = fq.FUSED_UPSAMPLE_FOREST
    for n_rays in args.rays:
        rt = rays_towards_hub(model, dev, n_rays)
        seg = [rt[k] for k in SEG_KEYS]
        for name, march_cfg in MARCH.items():
            key = f"{n_rays}_{name}"
            with torch.no_grad():
                marched = model.accel.ray_march(rt['rays_o'], rt['rays_d'], rt['near'], rt['far'], *seg, **march_cfg)
                depth, bl, pi, n_hit = marched.depth_samples.contiguous(), marched.blidx.contiguous(), marched.pack_infos, marched.num_hit_rays
                sdf = model.forward_sdf(marched.samples, bl)["sdf"].contiguous()
                shape = {"tested_rays": int(rt['num_rays']), "hit_rays": int(n_hit), "samples": int(depth.numel()),
                         "mean_pack": round(depth.numel() / max(n_hit, 1), 1), "max_pack": int(pi[:, 1].max()),
                         "blocks_marched": int(bl.unique().numel())}
                query = lambda: fq.neus_forest_ray_query_march_occ_multi_upsample(model, rt, march_cfg=march_cfg, **QUERY)   # noqa: E731
                model.sdf_block_inds.clear()
                (vb_f, _), bl_f = route(True, query)(), model.sdf_block_inds[-1]
                (vb_t, _), bl_t = route(False, query)(), model.sdf_block_inds[-1]

                def quiet():                                  # the model double keeps what it is given: not while timing
                    model.sdf_block_inds.clear()
                    return query()
                r = alternated({"fused": route(True, quiet), "chain": route(False, quiet)}, args.rounds, args.iters)
                r.update(shape, speedup=round(r["chain"]["ms"] / r["fused"]["ms"], 3),
                         max_abs_t_difference=(vb_f["t"] - vb_t["t"]).abs().max().item(), labels_differing=int((bl_f != bl_t).sum()),
                         labels=int(bl_f.numel()))
                res["queries"][key] = r
                print("query", key, shape, r["fused"]["ms"], r["chain"]["ms"], r["speedup"], r["max_abs_t_difference"],
                      r["labels_differing"], flush=True)
                u = torch.linspace(0., 1., 11, device=dev)[1:-1].contiguous()
                labelled = lambda: U.upsample_stage_packed_blocks(depth, sdf, bl, pi, u, 64.0, False)                         # noqa: E731
                plain = lambda: U.upsample_stage_packed(depth, sdf, pi, u, 64.0, False)                                       # noqa: E731
                a, b = labelled(), plain()
                assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[1]) and torch.equal(a[5], b[3]), "the two bindings compute the same"
                res["stage_alone"][key] = {}
                k_labelled, k_plain = stage_kernels(depth, sdf, bl, pi, u)
                for what, fns in (("kernel", {"labelled": k_labelled, "unlabelled": k_plain}),
                                  ("binding", {"labelled": labelled, "unlabelled": plain})):
                    r = alternated(fns, args.rounds, args.stage_iters)
                    r.update(overhead=round(r["labelled"]["ms"] / r["unlabelled"]["ms"], 3))
                    res["stage_alone"][key][what] = r
                    print("stage", what, key, r["labelled"]["ms"], r["unlabelled"]["ms"], r["overhead"], flush=True)
    fq.FUSED_UPSAMPLE_FOREST = default
    res["fused_below_chain_in_every_row"] = all(r["fused"]["ms"] < r["chain"]["ms"] for r in res["queries"].values())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
