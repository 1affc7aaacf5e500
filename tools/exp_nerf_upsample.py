#!/usr/bin/env python
"""tools/exp_nerf_upsample.py -- the packed stages of the NeRF march + up-sample query measured on one GPU -> profiles/nerf_upsample.json.

Workload: nerf_ray_query_march_occ_multi_upsample_compressed on an analytic density shell (so that the stages, not a network, are what
is timed) behind a 64^3 occupancy shell, 4096 and 65 536 rays, num_coarse = 32, num_fine = 32, unperturbed, no rgb, with two march step
sizes: packs of about 30 and of about 300 samples.  The fused route (FUSED_UPSAMPLE_NERF = True: one launch per stage) and the
pack-op chain (False) run in alternated rounds on the same inputs in one process; a round is the mean of ITERS queries (STAGE_ITERS
stage calls) between two events after a warm-up, the figure is the median of the rounds.  Also: the two stages alone (kernels against
the chain's ops, without the density queries), the largest |fused - chain| of the up-sampled depths, the launches per stage counted by
a `rocprofv3 --kernel-trace --stats` run of its own per route (--launches: child processes with 10 and 20 stage calls, the
difference over 10), and the same stages with the kernels built for each LDS row L in 256, 512, 1024 (--variants: csrc/nerf_upsample.hip
alone, compiled with -DNR3D_NERF_UPSAMPLE_LDS_ROW=L into csrc/build/variants/ and put in the library's place for the call; build them
beforehand with --build-variants where there is no GPU, which also writes the compiler's resource report of both kernels to
profiles/nerf_upsample_resources.txt).

    python tools/exp_nerf_upsample.py [--rays 4096 65536] [--rounds 7] [--iters 30] [--stage-iters 200] [--variants] [--launches]"""
import argparse
import ctypes
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

QUERY = dict(with_rgb=False, num_coarse=32, num_fine=32)
MARCH = {"packs_of_30": dict(step_size=0.03, max_steps=256), "packs_of_300": dict(step_size=0.003, max_steps=2048)}
VARIANTS = (256, 512, 1024)
VARIANT_DIR = os.path.join(ROOT, "nr3d_lib_amd", "csrc", "build", "variants")
ENTRIES = ("nr3d_nerf_merge_rows_packs", "nr3d_nerf_upsample_stage_packed", "nr3d_nerf_upsample_lds_row")
RESOURCES = os.path.join(ROOT, "profiles", "nerf_upsample_resources.txt")
HIPCC = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math"]


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
    return os.path.join(VARIANT_DIR, f"libnerf_upsample_L{L}.so")


def build_variants():
    from nr3d_lib_amd import _hip as H
    os.makedirs(VARIANT_DIR, exist_ok=True)
    pkg = os.path.dirname(H.LIB_PATH)
    report = []
    for L in VARIANTS:
        cmd = HIPCC + [f"-DNR3D_NERF_UPSAMPLE_LDS_ROW={L}", "-Rpass-analysis=kernel-resource-usage", "-shared",
                       os.path.join(H.CSRC, "nerf_upsample.hip"), "-o", variant_path(L), f"-L{pkg}", "-l:libnr3d_hip.so",
                       "-Wl,-rpath,$ORIGIN/../../.."]
        out = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
        report.append(f"== NR3D_NERF_UPSAMPLE_LDS_ROW = {L}{' (the library default)' if L == 512 else ''}")
        for line in out.splitlines():
            m = re.search(r"remark:\s+(Function Name: \S+|\s*(?:TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                          r"SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): \d+)", line)
            if m:
                report.append(("" if m.group(1).startswith("Function") else "    ") + m.group(1).strip())
        print("built", variant_path(L), flush=True)
    os.makedirs(os.path.dirname(RESOURCES), exist_ok=True)
    with open(RESOURCES, "w") as f:
        f.write("hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage csrc/nerf_upsample.hip\n"
                + "\n".join(report) + "\n")


class Variant:
    """the library's entries of this file replaced by those of the build for LDS row L while the block runs"""

    def __init__(self, L):
        from nr3d_lib_amd import _abi, _hip as H
        self.lib, self.var = H.lib(), ctypes.CDLL(variant_path(L))
        for name in ENTRIES:
            ret, args = _abi.SIGNATURES[name]
            fn = getattr(self.var, name)
            fn.restype, fn.argtypes = H._CTYPE[ret], [H._CTYPE[a] for a in args]
        assert int(self.var.nr3d_nerf_upsample_lds_row()) == L

    def __enter__(self):
        self.saved = {name: getattr(self.lib, name) for name in ENTRIES}
        for name in ENTRIES:
            setattr(self.lib, name, getattr(self.var, name))

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def density(x):
    return 4.0 * (1 + 0.48 * x[..., 2]) * torch.exp(-((x.norm(dim=-1) - 0.62) / 0.08) ** 2)


class ShellDensity(torch.nn.Module):
    def __init__(self, accel):
        super().__init__()
        self.accel = accel

    def query_density(self, x, **kw):
        return density(x)

    def forward_density(self, x, **kw):
        return dict(sigma=density(x))

    def forward(self, x, **kw):
        return dict(sigma=density(x), rgb=torch.sigmoid(x))


def scene(dev, n_rays, res=64):
    """the density shell behind an occupancy shell 0.45 < |x| < 0.8 and n_rays seeded rays from a pinhole at (0, 0, -4) towards it"""
    from demo_field import StaticOccGridAccel
    c = (torch.stack(torch.meshgrid(*[torch.arange(res)] * 3, indexing="ij"), -1) + 0.5) / res * 2 - 1
    r = c.norm(dim=-1)
    model = ShellDensity(StaticOccGridAccel(((r > 0.45) & (r < 0.8)).to(dev), 0.03)).eval()
    g = torch.Generator().manual_seed(0)
    d = torch.cat([0.2 * (torch.rand(n_rays, 2, generator=g) * 2 - 1), torch.ones(n_rays, 1)], -1)
    d = (d / d.norm(dim=-1, keepdim=True)).to(dev)
    o = torch.tensor([0.0, 0.0, -4.0]).repeat(n_rays, 1).to(dev)
    t1, t2 = (-1 - o) / d, (1 - o) / d
    near, far = torch.minimum(t1, t2).amax(1).clamp_min(0).contiguous(), torch.maximum(t1, t2).amin(1).contiguous()
    return model, dict(num_rays=n_rays, rays_o=o, rays_d=d, near=near, far=torch.maximum(far, near).contiguous(),
                       rays_inds=torch.arange(n_rays, device=dev))


class Stages:
    """the inputs of the two stages of one query (coarse rows, marched packs, the density at the merged samples) and both routes"""

    def __init__(self, model, rays, march_cfg, num_coarse, num_fine):
        from nr3d_lib_amd.bindings import _nerf_upsample as U
        from nr3d_lib_amd.graphics.nerf import nerf_ray_query as rq
        from nr3d_lib_amd.graphics.pack_ops import get_pack_infos_from_batch, get_pack_infos_from_n
        from nr3d_lib_amd.graphics.raysample import batch_sample_step_linear, cdf_positions
        self.U, self.nc, self.m = U, num_coarse, num_fine + 1
        self.o, self.d = rays["rays_o"].contiguous(), rays["rays_d"].contiguous()
        R, dev = self.o.shape[0], self.o.device
        marched = rq._march(model, rays, self.o, self.d, rays["near"], rays["far"], False, march_cfg)
        self.depth, self.pi_hit, self.hit, self.ridx = marched.depth_samples.view(-1).contiguous(), marched.pack_infos, marched.ridx_hit, marched.ridx
        t1, dt = batch_sample_step_linear(rays["near"], rays["far"], num_coarse + 1, return_dt=True)
        self.coarse = (t1[..., :num_coarse] + dt[..., :num_coarse] / 2.).contiguous()
        n = self.pi_hit.new_zeros(R)
        n[self.hit] = self.pi_hit[:, 1]
        self.pi_all, self.pi_coarse, self.all_rays = get_pack_infos_from_n(n), get_pack_infos_from_batch(R, num_coarse, device=dev), torch.arange(R, device=dev)
        self.u = cdf_positions(self.depth, (R,), self.m, False)
        a = self.fused_merge()
        self.sigma = density(a[3]).contiguous()
        self.shape = {"rays": R, "hit_rays": int(self.hit.numel()), "marched_samples": int(self.depth.numel()),
                      "mean_pack": round(self.depth.numel() / max(self.hit.numel(), 1), 1), "max_pack": int(self.pi_hit[:, 1].max())}

    def fused_merge(self):
        return self.U.merge_rows_packs(self.coarse, self.depth, self.pi_all, self.o, self.d)

    def fused(self):
        depths_all, deltas_all, _, _, pinfo = self.fused_merge()
        return self.U.upsample_stage_packed(depths_all, self.sigma, deltas_all, pinfo, self.u, coarse=self.coarse)

    def chain(self):
        """the pack-op chain of the driver between its density queries (without the queries)"""
        from nr3d_lib_amd.graphics.nerf.nerf_utils import tau_to_alpha
        from nr3d_lib_amd.graphics.pack_ops import (get_pack_infos_from_batch, merge_two_packs_sorted_a_includes_b, packed_cumsum,
                                                    packed_diff, packed_div)
        from nr3d_lib_amd.graphics.raysample import packed_sample_cdf
        nc, R = self.nc, self.o.shape[0]
        flat = self.coarse.flatten()
        pidx0, pidx1, pinfo = merge_two_packs_sorted_a_includes_b(flat, self.pi_coarse, self.all_rays, self.depth, self.pi_hit, self.hit, b_sorted=True)
        n = self.depth.numel() + flat.numel()
        depths_all, ridx_all = self.depth.new_zeros([n]), self.hit.new_zeros([n])
        ridx_all[pidx0], ridx_all[pidx1] = self.all_rays.unsqueeze(-1).expand(-1, nc).flatten(), self.ridx
        depths_all[pidx0], depths_all[pidx1] = flat, self.depth
        samples_all = torch.addcmul(self.o[ridx_all], self.d[ridx_all], depths_all.unsqueeze(-1))
        deltas_all = packed_diff(depths_all, pinfo)
        cdf = packed_cumsum(tau_to_alpha(self.sigma * deltas_all), pinfo)
        cdf = packed_div(cdf, cdf[pinfo[..., 0] + pinfo[..., 1] - 1].clamp_min(1e-5), pinfo)
        fine = packed_sample_cdf(depths_all, cdf, pinfo, self.m)[0]
        pinfo_fine = get_pack_infos_from_batch(R, self.m, device=fine.device)
        pidx0, pidx1, pinfo2 = merge_two_packs_sorted_a_includes_b(flat, self.pi_coarse, self.all_rays, fine.flatten(), pinfo_fine, self.all_rays,
                                                                   b_sorted=False)
        merged, ridx2 = fine.new_zeros([fine.numel() + flat.numel()]), self.hit.new_zeros([fine.numel() + flat.numel()])
        ridx2[pidx0], ridx2[pidx1] = self.all_rays.unsqueeze(-1).expand(-1, nc).flatten(), self.all_rays.unsqueeze(-1).expand(-1, self.m).flatten()
        merged[pidx0], merged[pidx1] = flat, fine.flatten()
        return fine, merged.view(R, nc + self.m), packed_diff(merged, pinfo2).view(R, nc + self.m)


def trace_child(route, n_rays, march, calls):
    """run under rocprofv3: `calls` stage calls of one route after the set-up, nothing else"""
    dev = torch.device("cuda:0")
    model, rays = scene(dev, n_rays)
    with torch.no_grad():
        st = Stages(model, rays, MARCH[march], QUERY["num_coarse"], QUERY["num_fine"])
        for _ in range(calls):
            getattr(st, route)()
    torch.cuda.synchronize()


def count_launches(n_rays, march):
    """{route: launches per stage call} from two traced child processes per route (10 and 20 calls)"""
    out = {}
    for route in ("fused", "chain"):
        totals = []
        for calls in (10, 20):
            with tempfile.TemporaryDirectory() as tmp:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                       "--trace", route, str(n_rays), march, str(calls)]
                subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
                n = 0
                for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
                    with open(path) as f:
                        n += sum(int(row["Calls"]) for row in csv.DictReader(f))
                totals.append(n)
        out[route] = (totals[1] - totals[0]) / 10
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--stage-iters", type=int, default=200, help="calls per round when the stages alone are timed")
    ap.add_argument("--variants", action="store_true", help="also time the stages with the kernels built for every LDS row")
    ap.add_argument("--launches", action="store_true", help="also count the launches per stage with rocprofv3 (child processes)")
    ap.add_argument("--build-variants", action="store_true", help="only compile the variant builds and write the resource report (needs no GPU)")
    ap.add_argument("--trace", nargs=4, metavar=("ROUTE", "RAYS", "MARCH", "CALLS"), help="internal: the traced child of --launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_upsample.json"))
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if args.trace:
        return trace_child(args.trace[0], int(args.trace[1]), args.trace[2], int(args.trace[3]))
    from nr3d_lib_amd.bindings import _nerf_upsample as U
    from nr3d_lib_amd.graphics.nerf import nerf_ray_query as rq
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "stage_iters": args.stage_iters,
           "lds_row": U.LDS_ROW, "query": dict(QUERY), "march": MARCH, "queries": {}, "stages_alone": {}, "launches_per_stage": {},
           "lds_row_variants": {}}

    def route(fused, fn):
        def run():
            rq.FUSED_UPSAMPLE_NERF = fused
            return fn()
        return run

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for n_rays in args.rays:
        model, rays = scene(dev, n_rays)
        for name, march_cfg in MARCH.items():
            key = f"{n_rays}_{name}"
            with torch.no_grad():
                st = Stages(model, rays, march_cfg, QUERY["num_coarse"], QUERY["num_fine"])
                query = lambda: rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, march_cfg=march_cfg, **QUERY)  # noqa: E731
                vb_f, vb_t = route(True, query)()[0], route(False, query)()[0]
                same = torch.equal(vb_f["rays_inds_hit"], vb_t["rays_inds_hit"]) and torch.equal(vb_f["pack_infos_hit"], vb_t["pack_infos_hit"])
                r = alternated({"fused": route(True, query), "chain": route(False, query)}, args.rounds, args.iters)
                r.update(st.shape, speedup=round(r["chain"]["ms"] / r["fused"]["ms"], 3), compressed_same_packs=bool(same),
                         compressed_samples={"fused": vb_f["t"].numel(), "chain": vb_t["t"].numel()})
                res["queries"][key] = r
                print("query", key, st.shape, r["fused"]["ms"], r["chain"]["ms"], r["speedup"], same, flush=True)
                f_out, c_out = st.fused(), st.chain()
                r = alternated({"fused": st.fused, "chain": st.chain}, args.rounds, args.stage_iters)
                r.update(speedup=round(r["chain"]["ms"] / r["fused"]["ms"], 3),
                         max_abs_fine_difference=(f_out[0] - c_out[0].sort(dim=-1).values).abs().max().item(),
                         max_abs_merged_difference=(f_out[1] - c_out[1]).abs().max().item())
                res["stages_alone"][key] = r
                print("stages", key, r["fused"]["ms"], r["chain"]["ms"], r["speedup"], r["max_abs_fine_difference"], flush=True)
                if args.variants:
                    fns = {}
                    for L in VARIANTS:
                        def with_variant(v=Variant(L)):
                            with v:
                                return st.fused()
                        fns[f"L{L}"] = with_variant
                    fns["library"] = st.fused
                    for k in ("L256", "L1024"):
                        assert all(torch.equal(a, b) for a, b in zip(fns[k](), f_out)), "the variants compute the same"
                    res["lds_row_variants"][key] = alternated(fns, args.rounds, args.stage_iters)
                    print("variants", key, {k: v["ms"] for k, v in res["lds_row_variants"][key].items()}, flush=True)
            save()
            if args.launches and not res["launches_per_stage"]:          # the count does not depend on the sizes: once
                res["launches_per_stage"][key] = count_launches(n_rays, name)
                print("launches", key, res["launches_per_stage"][key], flush=True)
                save()
    rq.FUSED_UPSAMPLE_NERF = True
    if os.path.exists(RESOURCES):
        with open(RESOURCES) as f:
            res["resources"] = f.read().splitlines()
    save()


if __name__ == "__main__":
    main()
