#!/usr/bin/env python
"""tools/exp_permuto.py -- times the permutohedral encoder (csrc/permuto*.hip) on
  * the reference's own workload (permuto/tests/compare_save_intermediate.py): 3,653,653 points, 7-D, 8 levels of 2 features,
    resolutions 16..2048, 2^16 tables, half parameters -- its comments give 4.77 / 14.48 / 9.96 / 18.90 ms for fwd / dL/dx /
    dL/dparam / double backward on an unnamed GPU (a published figure, not a same-box comparison);
  * the 3-D SDF configuration (get_permuto_cfg('multi_res') defaults: 16 levels 10..1000, 2 features, 2^19 tables) at 2^22 points,
    fp32 and half.
Four operations each: fwd, dL/dx alone, dL/dparam alone (zero fill and the cast to the table dtype included, as the reference's
call), double backward (both outputs).  Rounds alternate between the operations; each number is the median over rounds of the
mean of `--reps` back-to-back calls timed with events.  dL/dparam is also timed per level (a one-level meta of that level's
resolution over the same points).

    python tools/exp_permuto.py [--rounds 7] [--reps 5] [--out profiles/permuto_mi355x.json] [--quick]
    python tools/exp_permuto.py --counters   # one dL/dparam call of the reference workload, then of its levels 0 and 7 alone
                                             # (a one-level meta each), for a rocprofv3 --pmc run
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nr3d_lib_amd.bindings import _permuto as B  # noqa: E402
from nr3d_lib_amd.models.grid_encodings.permuto import get_permuto_cfg  # noqa: E402


def ops(meta, x, p, gy, ggx):
    return {
        "fwd": lambda: B.permuto_enc_fwd(meta, x, p),
        "dL_dx": lambda: B.permuto_enc_bwd(meta, gy, x, p, need_input_grad=True, need_param_grad=False),
        "dL_dparam": lambda: B.permuto_enc_bwd(meta, gy, x, p, need_input_grad=False, need_param_grad=True),
        "bwd_bwd": lambda: B.permuto_enc_bwd_bwd_input(meta, ggx, gy, x, p, need_dL_ddLdy=True, need_dL_dparams=True),
    }


def timed(fns, rounds, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {k: [] for k in fns}
    for f in fns.values():          # warm-up
        f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in fns.items():    # alternate the operations inside every round
            ev[0].record()
            for _ in range(reps):
                f()
            ev[1].record()
            torch.cuda.synchronize()
            res[k].append(ev[0].elapsed_time(ev[1]) / reps)
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), rounds=len(v))
            for k, v in res.items()}


def workload(D, res, nf, hs, N, dtype, rounds, reps, per_level):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    meta = B.PermutoEncMeta(D, hs, res, nf)
    x = torch.rand(N, D, device=dev, generator=g)
    p = torch.randn(meta.n_params, device=dev, generator=g).to(dtype)
    gy = torch.randn(N, meta.n_encoded_dims, device=dev, generator=g).to(dtype)
    ggx = torch.randn(N, D, device=dev, generator=g)
    out = dict(n_points=N, n_input_dim=D, res_list=[float(r) for r in res], n_feats_list=list(nf), hashmap_size=hs,
               param_dtype=str(dtype).replace("torch.", ""), timings=timed(ops(meta, x, p, gy, ggx), rounds, reps))
    if per_level:
        lv = []
        for l, r in enumerate(res):
            m1 = B.PermutoEncMeta(D, hs, [r], [nf[l]])
            p1 = p[meta.level_offsets[l]:meta.level_offsets[l + 1]].contiguous()
            gy1 = gy[:, sum(nf[:l]):sum(nf[:l + 1])].contiguous()
            t = timed({"dL_dparam": lambda: B.permuto_enc_bwd(m1, gy1, x, p1, need_input_grad=False, need_param_grad=True),
                       "fwd": lambda: B.permuto_enc_fwd(m1, x, p1)}, rounds, reps)
            lv.append(dict(level=l, res=float(r), dL_dparam_ms=t["dL_dparam"]["median_ms"], fwd_ms=t["fwd"]["median_ms"]))
        out["per_level"] = lv
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="one round, one rep, no per-level split (for a profiler run)")
    ap.add_argument("--counters", action="store_true", help="only the reference workload's dL/dparam: all levels, level 0, level 7")
    a = ap.parse_args()
    if a.counters:
        dev = torch.device("cuda:0")
        res = [16.0, 32.0, 64.0, 128.0, 256.0, 512.0, 1024.0, 2048.0]
        g = torch.Generator(device=dev).manual_seed(0)
        N = 3653653
        x = torch.rand(N, 7, device=dev, generator=g)
        gy = torch.randn(N, 16, device=dev, generator=g).half()
        for name, r, cols in (("all", res, slice(0, 16)), ("level0", res[:1], slice(0, 2)), ("level7", res[7:], slice(14, 16))):
            m = B.PermutoEncMeta(7, 2 ** 16, r, [2] * len(r))
            p = torch.zeros(m.n_params, device=dev, dtype=torch.half)
            B.permuto_enc_bwd(m, gy[:, cols].contiguous(), x, p, need_input_grad=False, need_param_grad=True)
            torch.cuda.synchronize()
            print("counters:", name, "done")
        return
    rounds, reps, per_level = (1, 1, False) if a.quick else (a.rounds, a.reps, True)
    t0 = time.time()
    ref_res = [16.0, 32.0, 64.0, 128.0, 256.0, 512.0, 1024.0, 2048.0]
    c = get_permuto_cfg("multi_res")
    rows = {
        "reference_7d_half": workload(7, ref_res, [2] * 8, 2 ** 16, 3653653, torch.float16, rounds, reps, per_level),
        "sdf_3d_fp32": workload(3, list(c["res_list"]), c["n_feats_list"], c["hashmap_size"], 2 ** 22, torch.float32, rounds, reps,
                                per_level),
        "sdf_3d_half": workload(3, list(c["res_list"]), c["n_feats_list"], c["hashmap_size"], 2 ** 22, torch.float16, rounds, reps,
                                False),
    }
    rows["reference_7d_half"]["reference_published_ms"] = dict(fwd=4.77, dL_dx=14.48, dL_dparam=9.96, bwd_bwd=18.90)
    doc = dict(device=torch.cuda.get_device_name(0), method=f"{rounds} alternating rounds x {reps} calls, median", workloads=rows,
               wall_s=round(time.time() - t0, 1))
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
