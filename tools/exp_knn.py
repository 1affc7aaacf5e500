#!/usr/bin/env python
"""tools/exp_knn.py -- ``maths.knn_points`` / ``chamfer_distance`` (csrc/knn.hip) measured on one GPU against the pure-torch route of the
same module (``FUSED_KNN = False``: explicit differences, chunked over P1, a stable sort per chunk) -> profiles/knn.json.  float32, D = 3,
standard normal points.

    chamfer   K = 1 in both directions at 2^14, 2^17 and 2^20 points per side
    lopsided  2^12 queries against 2^20 points, and 2^20 queries against 2^12 points (K = 1)
    knn       K = 8 and K = 16 at 2^17 per side
    generic   K = 40 at 2^14 per side (k_knn_any), and 2^15 .. 2^18 queries against 2^14 points: where the generic kernel overtakes the
              torch route, which is what ``GENERIC_MIN_ROWS`` is set from.  The "kernel" column of these rows is the kernel FORCED
              (``GENERIC_MIN_ROWS = 0``); ``default_route`` says what a caller gets

Per row: pairs per second, and from ``INNER_INSTRUCTIONS`` (the instructions of the kernel's inner loop per pair, read from the
disassembly: profiles/knn_resources.txt says how) the share of the FP32 vector peak that the rate implies -- instructions issued per
lane and second over the 78.65 T lane-instructions per second behind the 157.3 TFLOPS figure (which counts an FMA as two).  That share is
an ESTIMATE and an upper one of the VALU share: the table is entered by hand and counts every instruction of the loop block, the LDS
read, the waits and the loop control included; no counter is read (``share_note`` in the output says so too).

The two routes alternate; a round is the mean of as many calls as fill WINDOW_MS (at least one), a figure is the median of the rounds;
every call ends in a synchronise.  The torch route is measured where one call takes less than --torch-max-s seconds by the estimate from
a slice of its chunks; where it does not, the row says so with the estimate and is NOT shrunk.

    python tools/exp_knn.py [--rounds 5] [--out profiles/knn.json] [--rows chamfer_2^14 ...]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "knn.json")
WINDOW_MS = 250.0
FP32_VECTOR_TFLOPS = 157.3
# instructions per (query, point) pair in the inner loop of the kernel a row runs, from the disassembly (profiles/knn_resources.txt)
# (the path of a pair that does not enter the list: for K > 1 the insertion, 38 instructions at KB = 8 and 78 at KB = 16, is a branch)
INNER_INSTRUCTIONS = {"k_knn<3, 1, 2, 4>": 8.16, "k_knn<3, 1, 2, 1>": 13.9, "k_knn<3, 8, 2, 1>": 15.5, "k_knn<3, 16, 2, 1>": 15.5}

ROWS = [  # name, kind, P1, P2, K, kernel
    ("chamfer_2^14", "chamfer", 1 << 14, 1 << 14, 1, "k_knn<3, 1, 2, 1>"),
    ("chamfer_2^17", "chamfer", 1 << 17, 1 << 17, 1, "k_knn<3, 1, 2, 1>"),
    ("chamfer_2^20", "chamfer", 1 << 20, 1 << 20, 1, "k_knn<3, 1, 2, 4>"),
    ("knn_K1_2^12_vs_2^20", "knn", 1 << 12, 1 << 20, 1, "k_knn<3, 1, 2, 1>"),
    ("knn_K1_2^20_vs_2^12", "knn", 1 << 20, 1 << 12, 1, "k_knn<3, 1, 2, 4>"),
    ("knn_K8_2^17", "knn", 1 << 17, 1 << 17, 8, "k_knn<3, 8, 2, 1>"),
    ("knn_K16_2^17", "knn", 1 << 17, 1 << 17, 16, "k_knn<3, 16, 2, 1>"),
    ("knn_K40_2^14_generic", "knn", 1 << 14, 1 << 14, 40, "k_knn_any"),
    # the gate of the generic kernel (maths.pytorch3d_knn.GENERIC_MIN_ROWS): more query rows against the same 2^14 points
    ("generic_gate_2^15", "knn", 1 << 15, 1 << 14, 40, "k_knn_any"),
    ("generic_gate_2^16", "knn", 1 << 16, 1 << 14, 40, "k_knn_any"),
    ("generic_gate_2^17", "knn", 1 << 17, 1 << 14, 40, "k_knn_any"),
    ("generic_gate_2^18", "knn", 1 << 18, 1 << 14, 40, "k_knn_any"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--rows", nargs="*", default=None)
    ap.add_argument("--torch-max-s", type=float, default=4.0, help="skip the torch route of a row whose single call is estimated above this")
    ap.add_argument("--instructions", default=None, help="JSON {kernel: inner-loop instructions per pair} overriding INNER_INSTRUCTIONS")
    args = ap.parse_args()

    import torch
    from nr3d_lib_amd import maths
    from nr3d_lib_amd.maths import pytorch3d_knn as M
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    instr = dict(INNER_INSTRUCTIONS)
    gate = M.GENERIC_MIN_ROWS
    if args.instructions:
        instr.update(json.loads(args.instructions))

    def timed(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def call(kind, x, y, K, fused):
        def run():
            M.FUSED_KNN = fused
            M.GENERIC_MIN_ROWS = 0
            try:
                if kind == "chamfer":
                    return maths.chamfer_distance(x, y)
                return maths.knn_points(x, y, K=K)
            finally:
                M.FUSED_KNN, M.GENERIC_MIN_ROWS = True, gate
        return run

    def torch_estimate_s(kind, P1, P2):
        """one call of the torch route from a slice of its chunks (its cost is linear in the number of chunks)"""
        total = 0.0
        for a, b in ((P1, P2), (P2, P1)) if kind == "chamfer" else ((P1, P2),):
            rows = max(1, M.CHUNK_BYTES // (4 * b))
            n = min(a, 4 * rows)
            xs, ys = torch.randn(1, n, 3, device=dev), torch.randn(1, b, 3, device=dev)
            run = call("knn", xs, ys, 1, False)
            run()
            total += timed(run, 1) * 1e-3 * (a / n)
        return total

    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": WINDOW_MS, "dtype": "float32", "D": 3,
           "fp32_vector_tflops_assumed": FP32_VECTOR_TFLOPS, "torch_route_chunk_bytes": M.CHUNK_BYTES, "generic_min_rows": gate,
           "share_note": "share_of_fp32_vector_peak = pairs/s x hand-counted inner-loop instructions per pair (LDS read, waits and loop control "
                         "included) / 78.65e12: an upper estimate of the VALU share, not a counter reading",
           "rows": {}}
    g = torch.Generator(device=dev).manual_seed(0)
    for name, kind, P1, P2, K, kernel in ROWS:
        if args.rows and name not in args.rows:
            continue
        x, y = torch.randn(1, P1, 3, device=dev, generator=g), torch.randn(1, P2, 3, device=dev, generator=g)
        pairs = P1 * P2 * (2 if kind == "chamfer" else 1)
        routes = {"kernel": call(kind, x, y, K, True)}
        row = {"kind": kind, "P1": P1, "P2": P2, "K": K, "pairs_per_call": pairs, "kernel_name": kernel,
               "default_route": "kernel" if M._fused(x, K) else "torch"}
        est = torch_estimate_s(kind, P1, P2)
        row["torch_route_estimate_s"] = round(est, 3)
        if est <= args.torch_max_s:
            routes["torch"] = call(kind, x, y, K, False)
        else:
            row["torch_ms"] = None
            row["torch_note"] = (f"not measured: one call of the torch route is estimated at {est:.1f} s from a slice of its chunks "
                                 f"(it fits in memory, {M.CHUNK_BYTES >> 20} MiB per chunk, but not in the time of a measurement); the row is not shrunk")
        iters = {}
        for k, fn in routes.items():
            fn()
            iters[k] = max(1, min(1000, int(WINDOW_MS / max(timed(fn, 1), 1e-3)) + 1))
        t = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                t[k].append(timed(fn, iters[k]))
        for k, v in t.items():
            row[f"{k}_ms"] = round(statistics.median(v), 4)
            row[f"{k}_rounds_ms"] = [round(a, 4) for a in v]
        row["iters"] = iters
        rate = pairs / (row["kernel_ms"] * 1e-3)
        row["kernel_pairs_per_s"] = float(f"{rate:.4g}")
        if row.get("torch_ms"):
            row["torch_pairs_per_s"] = float(f"{pairs / (row['torch_ms'] * 1e-3):.4g}")
            row["torch_over_kernel"] = round(row["torch_ms"] / row["kernel_ms"], 2)
            a, b = routes["kernel"](), routes["torch"]()
            da, db = (a if kind == "chamfer" else (a.dists,)), (b if kind == "chamfer" else (b.dists,))
            row["routes_max_abs_dist_diff"] = float(max((p - q).abs().max().item() for p, q in zip(da, db)))
            if kind != "chamfer":       # the torch route rounds the squares before it adds them: near ties may come in the other order
                row["routes_idx_mismatches"] = int((a.idx != b.idx).sum().item())
        else:
            row["kernel_over_torch_estimate"] = round(est * 1e3 / row["kernel_ms"], 1)
        if instr.get(kernel):
            row["inner_loop_instructions_per_pair"] = instr[kernel]
            row["share_of_fp32_vector_peak"] = round(rate * instr[kernel] / (FP32_VECTOR_TFLOPS * 1e12 / 2), 4)
        res["rows"][name] = row
        print(name, {k: v for k, v in row.items() if not k.endswith("rounds_ms")}, flush=True)
        del x, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
