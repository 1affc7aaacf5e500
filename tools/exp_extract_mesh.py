#!/usr/bin/env python
"""tools/exp_extract_mesh.py -- mesh extraction (graphics.trianglemesh over csrc/marching_cubes.hip) measured on one GPU ->
profiles/extract_mesh.json.  There is nothing to compare with on the GPU (the reference's route is skimage on the host, which this
project's interpreter does not have), so these are figures, not a verdict.

    kernels    analytic sphere and torus at 128^3, 256^3, 512^3: the count entry (row counts + both scans: device time between two events),
               the count entry with its host wait (host clock: the ONE readback of an extraction), the emit entry (device time); the
               volume's bytes over the count kernel+scans time as a fraction of the 8 TB/s HBM rate, for information (the kernel reads a
               row nine times, from cache)
    pipeline   ``extract_mesh_tensors`` dense against sparse (a 64^3 occupancy of the shell around the surface) at 256^3 with a LoTD16 +
               MLP(35 -> 64 -> 1) of random weights as a small perturbation of an analytic sphere, split into query and triangulation
    restatement baseline   tests/marching_cubes_ref.py (numpy, one core) at 128^3 on the host -- NOT the reference's route

The measured calls alternate; a round is the mean of as many calls as fill WINDOW_MS (at least 3), a figure is the median of the rounds;
every shape is warmed first.

    python tools/exp_extract_mesh.py [--rounds 7] [--out profiles/extract_mesh.json] [--sizes 128 256 512] [--kernels-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "extract_mesh.json")
HBM_BYTES_PER_S = 8.0e12
WINDOW_MS = 100.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--pipeline-n", type=int, default=256)
    ap.add_argument("--kernels-only", action="store_true", help="the kernel rows alone (A/B of two builds of the library)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from nr3d_lib_amd import _hip as H
    from nr3d_lib_amd.bindings import _marching_cubes as B
    from nr3d_lib_amd.graphics import trianglemesh as TM
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")

    def sphere(x):
        return torch.sqrt((x * x).sum(-1)) - 0.6

    def torus(x):
        q = torch.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2) - 0.55
        return torch.sqrt(q * q + x[..., 2] ** 2) - 0.22

    def volume(fn, n):
        g = torch.linspace(-1, 1, n, device=dev)
        out = torch.empty((n, n, n), device=dev)
        for i in range(n):                                    # a slab at a time: no [n^3, 3] tensor
            out[i] = fn(torch.stack(torch.meshgrid(g[i:i + 1], g, g, indexing="ij"), -1))[0]
        return out

    def events(fn, iters=1):
        """device time per call of `iters` calls between two events"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    def host(fn, iters=1):
        """host time per call of `iters` calls that each end in their own device wait"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return (time.perf_counter() - t0) * 1e3 / iters

    def iters_for(ms):
        return max(3, min(2000, int(WINDOW_MS / max(ms, 1e-3)) + 1))

    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": WINDOW_MS, "kernels": {}, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S}
    l = H.lib()
    for n in args.sizes:
        for name, fn in (("sphere", sphere), ("torus", torus)):
            vol = volume(fn, n)
            st = H.stream_of(vol)
            scratch = torch.empty((int(l.nr3d_marching_cubes_scratch_bytes(n, n, n)) + 7) // 8, dtype=torch.int64, device=dev)
            totals_dev = torch.zeros(2, dtype=torch.int64, device=dev)

            def count_dev():
                H.check(l.nr3d_marching_cubes_count(H.ptr(vol), n, n, n, 0.0, H.ptr(scratch), H.ptr(totals_dev), st))

            def count_wait():
                totals = H.host_i64(2, dev)
                H.check(l.nr3d_marching_cubes_count(H.ptr(vol), n, n, n, 0.0, H.ptr(scratch), H.ptr(totals), st))
                return H.wait_i64(totals, dev)

            V, F = count_wait()
            verts = torch.empty((V, 3), device=dev)
            faces = torch.empty((F, 3), dtype=torch.int64, device=dev)

            def emit():
                H.check(l.nr3d_marching_cubes_emit(H.ptr(vol), n, n, n, 0.0, H.ptr(scratch), V, F, H.ptr(verts), H.ptr(faces), st))

            def whole():
                B.marching_cubes(vol, 0.0)
                torch.cuda.synchronize()

            for _ in range(3):
                count_dev(), count_wait(), emit(), whole()
            torch.cuda.synchronize()
            fns = {"count_scans_device_ms": (events, count_dev), "count_scans_wait_host_ms": (host, count_wait),
                   "emit_device_ms": (events, emit), "whole_call_host_ms": (host, whole)}
            iters = {k: iters_for(timer(call, 5)) for k, (timer, call) in fns.items()}
            t = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, (timer, call) in fns.items():
                    t[k].append(timer(call, iters[k]))
            row = {k: round(statistics.median(v), 4) for k, v in t.items()}
            row.update(V=V, F=F, scratch_bytes=int(scratch.numel() * 8), volume_bytes=int(vol.numel() * 4),
                       volume_bytes_over_count_time_fraction_of_hbm=round(vol.numel() * 4 / (row["count_scans_device_ms"] * 1e-3) / HBM_BYTES_PER_S, 4),
                       iters=iters, rounds={k: [round(x, 4) for x in v] for k, v in t.items()})
            res["kernels"][f"{name} {n}^3"] = row
            print(f"{name} {n}^3", {k: v for k, v in row.items() if k != "rounds"}, flush=True)
            del vol, scratch, verts, faces
            torch.cuda.empty_cache()

    if args.kernels_only:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return

    # ---- the pipeline: dense against sparse with a network query
    from nr3d_lib_amd.models.blocks import MLP
    from nr3d_lib_amd.models.grid_encodings.lotd import LoTDEncoding, gen_ngp_cfg
    cfg = gen_ngp_cfg(num_levels=16)
    torch.manual_seed(0)
    enc = LoTDEncoding(3, lotd_cfg=dict(lod_res=cfg["lod_res"], lod_n_feats=cfg["lod_n_feats"], lod_types=cfg["lod_types"],
                                        hashmap_size=cfg["hashmap_size"]), dtype=torch.float, device=dev)
    dec = MLP(35, 1, D=1, W=64, dtype=torch.float, device=dev)
    clock = {"query_ms": 0.0}

    def net_sdf(x):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = x.contiguous()
        out = sphere(x) + 0.005 * torch.tanh(dec(torch.cat([enc(x.clamp(-1, 1)), x], dim=-1))[..., 0])
        torch.cuda.synchronize()
        clock["query_ms"] += (time.perf_counter() - t0) * 1e3
        return out

    n = args.pipeline_n
    R = 64
    c = (torch.arange(R, device=dev) + 0.5) / R * 2 - 1
    centres = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1)
    occ = (sphere(centres).abs() <= 0.5 * (2 / R) * 3 ** 0.5 + 0.005)
    kw = dict(level=0.0, N=n, chunk=1 << 20, show_progress=False, device=dev)

    def run(sparse):
        clock["query_ms"] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh = TM.extract_mesh_tensors(net_sdf, occ_grid=occ if sparse else None, occ_aabb=[[-1., -1, -1], [1., 1, 1]] if sparse else None, **kw)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        return mesh, total, clock["query_ms"]

    d, s = run(False)[0], run(True)[0]
    same = bool(torch.equal(d["verts"], s["verts"]) and torch.equal(d["faces"], s["faces"]))
    rows = {"dense": [], "sparse": []}
    for _ in range(args.rounds):
        for key, sparse in (("dense", False), ("sparse", True)):
            _, total, q = run(sparse)
            rows[key].append((total, q))
    pipe = {"grid": [n, n, n], "occupancy": f"{R}^3, {int(occ.sum())} voxels occupied", "chunk": kw["chunk"], "sparse_equals_dense": same,
            "dense_stats": d["stats"], "sparse_stats": s["stats"]}
    for key, v in rows.items():
        total, q = statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)
        pipe[key] = {"total_ms": round(total, 3), "query_ms": round(q, 3), "rest_ms": round(total - q, 3),
                     "total_rounds_ms": [round(x[0], 3) for x in v]}
    res["pipeline"] = pipe
    print("pipeline", pipe, flush=True)

    # ---- the numpy restatement on the host at 128^3: a labelled baseline, not the reference
    import marching_cubes_ref as ref
    v128 = volume(sphere, 128).cpu().numpy()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        rv, rf = ref.marching_cubes(v128, 0.0)
        ts.append((time.perf_counter() - t0) * 1e3)
    gv, gf = B.marching_cubes(torch.from_numpy(v128).to(dev), 0.0)
    res["restatement_baseline"] = {"what": "tests/marching_cubes_ref.py (numpy, host) on the sphere at 128^3; not the reference's route",
                                   "ms": round(statistics.median(ts), 2), "V": int(len(rv)), "F": int(len(rf)),
                                   "equal_to_kernel": bool(np.array_equal(gv.cpu().numpy(), rv) and np.array_equal(gf.cpu().numpy(), rf))}
    print("restatement baseline", res["restatement_baseline"], flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
