#!/usr/bin/env python
"""tools/exp_neus_upsample_packed.py -- the packed NeuS up-sampling stage measured on one GPU -> profiles/neus_upsample_packed.json.

Workload: neus_ray_query_march_occ_multi_upsample_compressed on an analytic sphere SDF (so that the stages, not a network, are what
is timed) behind a 64^3 occupancy shell, 4096 and 65 536 rays, num_fine = 8, factors [1, 4, 16], unperturbed, no rgb / normals, with
two march step sizes: packs of about 30 and of about 300 samples.  The fused route (FUSED_UPSAMPLE_PACKED = True: one launch per
stage) and the pack-op chain (False: the code as it was) run in alternated rounds on the same inputs; a round is the mean of ITERS
queries (STAGE_ITERS stage calls) between two events after a warm-up, the figure is the median of the rounds.  Also: the first stage
alone (kernel against the chain's ops, without the SDF query), the largest |fused - chain| of the query's depths, and the same stage with the kernel
built for each LDS row L in 256, 512, 1024 (--variants: csrc/neus_upsample.hip alone, compiled with
-DNR3D_NEUS_UPSAMPLE_PACKED_LDS_ROW=L into csrc/build/variants/ and put in the library's place for the call; build them beforehand with
--build-variants where there is no GPU).

    python tools/exp_neus_upsample_packed.py [--rays 4096 65536] [--rounds 7] [--iters 50] [--stage-iters 500] [--variants] [--out profiles/...json]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

QUERY = dict(with_rgb=False, with_normal=False, num_coarse=0, num_fine=8, upsample_inv_s_factors=[1, 4, 16])
MARCH = {"packs_of_30": dict(step_size=0.03, max_steps=256), "packs_of_300": dict(step_size=0.003, max_steps=2048)}
VARIANTS = (256, 512, 1024)
VARIANT_DIR = os.path.join(ROOT, "nr3d_lib_amd", "csrc", "build", "variants")
ENTRIES = ("nr3d_neus_upsample_stage_packed", "nr3d_neus_upsample_packed_lds_row")


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


def variant_path(L):
    return os.path.join(VARIANT_DIR, f"libneus_upsample_L{L}.so")


def build_variants():
    from nr3d_lib_amd import _hip as H
    os.makedirs(VARIANT_DIR, exist_ok=True)
    pkg = os.path.dirname(H.LIB_PATH)
    for L in VARIANTS:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
               f"-DNR3D_NEUS_UPSAMPLE_PACKED_LDS_ROW={L}", "-shared", os.path.join(H.CSRC, "neus_upsample.hip"), "-o", variant_path(L),
               f"-L{pkg}", "-l:libnr3d_hip.so", "-Wl,-rpath,$ORIGIN/../../.."]
        subprocess.check_call(cmd)
        print("built", variant_path(L), flush=True)


class Variant:
    """the library's two packed entries replaced by those of the build for LDS row L while the block runs"""

    def __init__(self, L):
        from nr3d_lib_amd import _abi, _hip as H
        self.lib, self.var = H.lib(), ctypes.CDLL(variant_path(L))
        for name in ENTRIES:
            ret, args = _abi.SIGNATURES[name]
            fn = getattr(self.var, name)
            fn.restype, fn.argtypes = H._CTYPE[ret], [H._CTYPE[a] for a in args]
        assert int(self.var.nr3d_neus_upsample_packed_lds_row()) == L

    def __enter__(self):
        self.saved = {name: getattr(self.lib, name) for name in ENTRIES}
        for name in ENTRIES:
            setattr(self.lib, name, getattr(self.var, name))

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def scene(dev, n_rays, res=64):
    """the sphere behind an occupancy shell 0.45 < |x| < 0.8 and n_rays seeded rays from a pinhole at (0, 0, -4) towards it"""
    import neus_coarse_ref as cref
    from demo_field import StaticOccGridAccel
    c = (torch.stack(torch.meshgrid(*[torch.arange(res)] * 3, indexing="ij"), -1) + 0.5) / res * 2 - 1
    r = c.norm(dim=-1)
    model = cref.SphereModel()
    model.accel = StaticOccGridAccel(((r > 0.45) & (r < 0.8)).to(dev), 0.03)
    model.eval()
    g = torch.Generator().manual_seed(0)
    d = torch.cat([0.2 * (torch.rand(n_rays, 2, generator=g) * 2 - 1), torch.ones(n_rays, 1)], -1)
    d = (d / d.norm(dim=-1, keepdim=True)).to(dev)
    o = torch.tensor([0.0, 0.0, -4.0]).repeat(n_rays, 1).to(dev)
    t1, t2 = (-1 - o) / d, (1 - o) / d
    near, far = torch.minimum(t1, t2).amax(1).clamp_min(0).contiguous(), torch.maximum(t1, t2).amin(1).contiguous()
    return model, dict(num_rays=n_rays, rays_o=o, rays_d=d, near=near, far=torch.maximum(far, near).contiguous(),
                       rays_inds=torch.arange(n_rays, device=dev))


def chain_stage(depth, sdf, pack_infos, n_packs, m, inv_s):
    """one stage of the pack-op chain as _packed_upsample.upsample_loop runs it between two SDF queries (without the query)"""
    from nr3d_lib_amd.graphics.neus.neus_utils import neus_packed_sdf_to_alpha
    from nr3d_lib_amd.graphics.pack_ops import (get_pack_infos_from_batch, merge_two_packs_sorted_aligned, packed_alpha_to_vw,
                                                packed_cumsum, packed_div)
    from nr3d_lib_amd.graphics.raysample import packed_sample_cdf
    cdf = packed_cumsum(packed_alpha_to_vw(neus_packed_sdf_to_alpha(sdf, inv_s, pack_infos), pack_infos), pack_infos, exclusive=True)
    cdf = packed_div(cdf, cdf[pack_infos[..., 0] + pack_infos[..., 1] - 1].clamp_min(1e-5), pack_infos)
    fine = packed_sample_cdf(depth, cdf, pack_infos, m)[0]
    pidx0, pidx1, pinfo = merge_two_packs_sorted_aligned(depth, pack_infos, fine.flatten(), get_pack_infos_from_batch(n_packs, m, device=depth.device),
                                                         b_sorted=True, return_val=False)
    merged, sdf_m = depth.new_empty(depth.numel() + fine.numel()), sdf.new_empty(depth.numel() + fine.numel())
    merged[pidx0], merged[pidx1] = depth, fine.flatten()
    sdf_m[pidx0] = sdf
    return fine, merged, sdf_m, pidx1, pinfo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--stage-iters", type=int, default=500, help="calls per round when one stage alone is timed")
    ap.add_argument("--variants", action="store_true", help="also time the stage with the kernel built for every LDS row")
    ap.add_argument("--build-variants", action="store_true", help="only compile the variant builds (needs no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neus_upsample_packed.json"))
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    from nr3d_lib_amd.bindings import _neus_upsample as U
    from nr3d_lib_amd.graphics.neus import neus_ray_query as rq
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "stage_iters": args.stage_iters, "lds_row": U.PACKED_LDS_ROW,
           "query": dict(QUERY), "march": MARCH, "queries": {}, "stage_alone": {}, "lds_row_variants": {}}

    def route(fused, fn):
        def run():
            rq.FUSED_UPSAMPLE_PACKED = fused
            return fn()
        return run

    for n_rays in args.rays:
        model, rays = scene(dev, n_rays)
        for name, march_cfg in MARCH.items():
            key = f"{n_rays}_{name}"
            with torch.no_grad():
                marched = rq._march(model, rays, rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], False, march_cfg)
                depth, pi, n_hit = marched.depth_samples.contiguous(), marched.pack_infos, marched.num_hit_rays
                sdf = model.forward_sdf(marched.samples)["sdf"].contiguous()
                shape = {"hit_rays": int(n_hit), "samples": int(depth.numel()), "mean_pack": round(depth.numel() / max(n_hit, 1), 1),
                         "max_pack": int(pi[:, 1].max())}
                query = lambda: rq.neus_ray_query_march_occ_multi_upsample_compressed(model, rays, march_cfg=march_cfg, **QUERY)  # noqa: E731
                # the depths of the two routes, before the compression (a threshold on them: a last-bit difference can move a sample
                # across it, so the compressed packs are compared by count)
                plain = lambda: rq.neus_ray_query_march_occ_multi_upsample(model, rays, march_cfg=march_cfg, **QUERY)[0]["t"]   # noqa: E731
                t_f, t_t = route(True, plain)(), route(False, plain)()
                vb_f, vb_t = route(True, query)()[0], route(False, query)()[0]
                same_rays = torch.equal(vb_f["rays_inds_hit"], vb_t["rays_inds_hit"])
                r = alternated({"fused": route(True, query), "chain": route(False, query)}, args.rounds, args.iters)
                r.update(shape, speedup=round(r["chain"]["ms"] / r["fused"]["ms"], 3), max_abs_t_difference=(t_f - t_t).abs().max().item(),
                         compressed_samples={"fused": vb_f["t"].numel(), "chain": vb_t["t"].numel()}, compressed_same_rays=bool(same_rays),
                         compressed_packs_differing=int((vb_f["pack_infos_hit"][:, 1] != vb_t["pack_infos_hit"][:, 1]).sum()) if same_rays else None)
                res["queries"][key] = r
                print("query", key, shape, r["fused"]["ms"], r["chain"]["ms"], r["speedup"], r["max_abs_t_difference"], r["compressed_samples"],
                      r["compressed_packs_differing"], flush=True)
                u = torch.linspace(0., 1., 11, device=dev)[1:-1].contiguous()
                fused_stage = lambda: U.upsample_stage_packed(depth, sdf, pi, u, 64.0, False)                                  # noqa: E731
                r = alternated({"fused": fused_stage, "chain": lambda: chain_stage(depth, sdf, pi, n_hit, 9, 64.0)}, args.rounds, args.stage_iters)
                r.update(speedup=round(r["chain"]["ms"] / r["fused"]["ms"], 3),
                         max_abs_fine_difference=(fused_stage()[0] - chain_stage(depth, sdf, pi, n_hit, 9, 64.0)[0]).abs().max().item())
                res["stage_alone"][key] = r
                print("stage", key, r["fused"]["ms"], r["chain"]["ms"], r["speedup"], r["max_abs_fine_difference"], flush=True)
                if args.variants:
                    fns = {}
                    for L in VARIANTS:
                        def with_variant(v=Variant(L)):
                            with v:
                                return fused_stage()
                        fns[f"L{L}"] = with_variant
                    fns["library"] = fused_stage
                    base = fused_stage()
                    got = fns["L256"]()
                    assert all(torch.equal(got[i], base[i]) for i in (0, 1, 3, 4)), "the variants compute the same"
                    res["lds_row_variants"][key] = alternated(fns, args.rounds, args.stage_iters)
                    print("variants", key, {k: v["ms"] for k, v in res["lds_row_variants"][key].items()}, flush=True)
    rq.FUSED_UPSAMPLE_PACKED = True
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
