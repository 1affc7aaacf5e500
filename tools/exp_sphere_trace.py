#!/usr/bin/env python
"""tools/exp_sphere_trace.py -- the sphere tracer on 512 x 512 rays through a 128^3 occupancy grid (graphics/sphere_trace.py).

Two distance functions: (i) an analytic sphere (radius 0.5), (ii) the same sphere displaced by a 16-level LoTD encoding + MLP(35 -> 64 -> 1)
(the SDF network of tools/exp_mlp_second_order.py, untrained: 0.02 * tanh(net) keeps the surface a perturbed sphere; the query costs
what a trained network's would).  Per scene: ms per trace (median of --reps after --warmup), steps taken, tracer launches per step
between compactions, host waits per trace, and the wall-time split tracer calls / SDF queries / host waits (host timers around each
call with a device synchronisation, in a separate run from the headline time, which has none).
    python tools/exp_sphere_trace.py [--reps R] [--warmup W] [--side 512] [--out FILE.json] [--once SCENE]
``--once SCENE`` runs one warm trace of one scene and exits: the program for `rocprofv3 --kernel-trace --stats -- ...`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nr3d_lib_amd import _hip as H
from nr3d_lib_amd.bindings import _sphere_trace as B
from nr3d_lib_amd.graphics.sphere_trace import DenseGrid, SphereTracer


def scene(dev, side, res=128):
    c = (torch.arange(res, device=dev, dtype=torch.float32) + 0.5) / res * 2 - 1
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    grid = (torch.sqrt(X * X + Y * Y + Z * Z) < 0.5 + 0.03 + 2 * 3 ** 0.5 / res).contiguous()
    u = torch.linspace(-0.7, 0.7, side, device=dev)
    U, V = torch.meshgrid(u, u, indexing="ij")
    d = torch.nn.functional.normalize(torch.stack([U.reshape(-1), V.reshape(-1), torch.ones(side * side, device=dev)], -1), dim=-1)
    o = torch.tensor([0., 0., -0.95], device=dev).repeat(side * side, 1)
    rays = dict(rays_o=o.contiguous(), rays_d=d.contiguous(), near=torch.zeros(side * side, device=dev),
                far=torch.full((side * side,), 3.0, device=dev))
    return DenseGrid(res, res, res, grid), rays


def sphere(x):
    return torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]) - 0.5


def network_sdf(dev):
    from nr3d_lib_amd.models.blocks import MLP
    from nr3d_lib_amd.models.grid_encodings.lotd import LoTDEncoding, gen_ngp_cfg
    cfg = gen_ngp_cfg(num_levels=16)
    torch.manual_seed(0)
    enc = LoTDEncoding(3, lotd_cfg=dict(lod_res=cfg["lod_res"], lod_n_feats=cfg["lod_n_feats"], lod_types=cfg["lod_types"],
                                        hashmap_size=cfg["hashmap_size"]), dtype=torch.float, device=dev)
    dec = MLP(35, 1, D=1, W=64, dtype=torch.float, device=dev)

    def sdf(x):
        x = x.contiguous()
        h = enc(x.clamp(-1, 1))
        return sphere(x) + 0.02 * torch.tanh(dec(torch.cat([h, x], dim=-1))[..., 0])
    return sdf


class Counted:
    """wraps the backend's calls: counts them, and (timed=True) brackets each with a device synchronisation and a host timer"""
    TRACER = ("init_rays", "advance_rays", "compact_rays", "get_rays", "sample_on_segments", "trace_on_samples")

    def __init__(self, tracer, timed):
        self.n, self.ms, self.timed = {}, {}, timed
        for name in self.TRACER:
            setattr(tracer.backend, name, self.wrap(name, getattr(tracer.backend, name)))

    def wrap(self, name, fn):
        def call(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            if not self.timed:
                return fn(*a, **k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return r
        return call


def run(name, grid, rays, sdf, reps, warmup):
    tracer = SphereTracer(grid, min_step=0.01, hit_threshold=1e-3)

    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tracer.trace(rays, sdf)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(warmup):
        once()
    times = sorted(once()[0] for _ in range(reps))
    out = once()[1]
    # the split: one run with every backend call and every SDF query bracketed; waits counted through _hip.wait_i64
    waits = dict(n=0, ms=0.0)
    real_wait = H.wait_i64

    def wait(buf, dev):
        t0 = time.perf_counter()
        r = real_wait(buf, dev)
        waits["n"] += 1
        waits["ms"] += (time.perf_counter() - t0) * 1e3
        return r

    q = dict(n=0, ms=0.0)

    def timed_sdf(x):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = sdf(x)
        torch.cuda.synchronize()
        q["n"] += 1
        q["ms"] += (time.perf_counter() - t0) * 1e3
        return r

    tracer2 = SphereTracer(grid, min_step=0.01, hit_threshold=1e-3)
    cnt = Counted(tracer2, timed=True)
    real_march = B.ray_march
    H.wait_i64, B.ray_march = wait, cnt.wrap("ray_march", real_march)
    try:
        tracer2.trace(rays, timed_sdf)
    finally:
        H.wait_i64, B.ray_march = real_wait, real_march
    steps, compactions = cnt.n.get("advance_rays", 0), cnt.n.get("compact_rays", 0)
    return dict(scene=name, rays=int(rays["rays_o"].shape[0]), hits=int(out["idx"].numel()), ms_per_trace=round(times[len(times) // 2], 3),
                ms_min=round(times[0], 3), ms_max=round(times[-1], 3), steps=steps, compactions=compactions,
                tracer_launches_per_step=1, sdf_queries=q["n"], host_waits_per_trace=waits["n"],
                host_waits_expected=compactions + 1,
                split_ms=dict(tracer_calls=round(sum(cnt.ms.values()) - waits["ms"], 3), sdf_queries=round(q["ms"], 3),
                              host_waits=round(waits["ms"], 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", default=None, choices=["sphere", "network"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    grid, rays = scene(dev, args.side)
    scenes = dict(sphere=sphere, network=network_sdf(dev))
    if args.once:
        tracer = SphereTracer(grid, min_step=0.01, hit_threshold=1e-3)
        for _ in range(2):
            out = tracer.trace(rays, scenes[args.once])
        torch.cuda.synchronize()
        print(json.dumps(dict(scene=args.once, hits=int(out["idx"].numel()), steps=tracer.last_march_iters)))
        return
    rows = []
    for name, sdf in scenes.items():
        rows.append(run(name, grid, rays, sdf, args.reps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), grid=128, reps=args.reps, warmup=args.warmup, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
