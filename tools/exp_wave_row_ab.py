#!/usr/bin/env python
"""tools/exp_wave_row_ab.py OTHER_LIB [OUT.json] -- the NeuS up-sampling stages (the kernels of neus_upsample.hip, the one object whose
machine code csrc/wave_row.h changed) timed on this tree's libnr3d_hip.so and on OTHER_LIB, another build of the same ABI (the parent
commit's), IN ONE PROCESS -> profiles/wave_row.md.

Both libraries are loaded with ctypes; ``_hip._lib`` is switched between them, so the same bindings, inputs and allocator serve both.
Per entry: the outputs of the two are compared first (``same_bits``), then ROUNDS rounds per library, alternating and reversing the
order every round, each the mean of as many calls between two events as fill about WINDOW_MS.  Reported: the median and the range of
the rounds.  Separate processes of the same code differ by percents on this workload (profiles/wave_row.md); rounds alternating inside
one process do not."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, WINDOW_MS = 9, 120.0


def main():
    import torch
    from nr3d_lib_amd import _hip
    from nr3d_lib_amd.bindings import _neus_upsample
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    other = C.CDLL(os.path.abspath(sys.argv[1]))
    assert int(other.nr3d_abi_version()) == _hip.ABI_VERSION, "the other library has another ABI"
    _hip._declare(other)
    libs = {"other": other, "this": _hip.lib()}
    gen = torch.Generator().manual_seed(0)
    res = {}

    def timed(fn, iters):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    def case(name, fn, pick=lambda out: out):
        outs = {}
        for k, l in libs.items():
            _hip._lib = l
            outs[k] = [t.clone() for t in pick(fn()) if t is not None]
        same = all(torch.equal(a, b) for a, b in zip(outs["other"], outs["this"]))
        iters = max(20, int(WINDOW_MS / timed(fn, 20)))
        t = {k: [] for k in libs}
        for r in range(ROUNDS):
            for k in (list(libs) if r % 2 == 0 else list(libs)[::-1]):
                _hip._lib = libs[k]
                fn()
                t[k].append(timed(fn, iters))
        _hip._lib = libs["this"]
        res[name] = {"same_bits": same, "iters": iters, **{f"{k}_ms": round(statistics.median(v), 5) for k, v in t.items()},
                     **{f"{k}_range_ms": [round(min(v), 5), round(max(v), 5)] for k, v in t.items()}}
        print(name, res[name], flush=True)

    for P, mean in ((4096, 30), (4096, 300), (65536, 30), (65536, 300)):       # packs as a marcher's: lengths in [mean / 2, 3 mean / 2]
        lens = torch.randint(mean // 2, mean * 3 // 2 + 1, (P,), generator=gen)
        first, rep = lens.cumsum(0) - lens, lens.repeat_interleave(lens)
        within = torch.arange(int(lens.sum())) - first.repeat_interleave(lens)
        d = (0.5 + 3.0 * (within + torch.rand(within.shape, generator=gen) * 0.9) / rep).float().contiguous().to(dev)
        pi, sdf = torch.stack([first, lens], 1).contiguous().to(dev), (2.0 - d).contiguous()
        u = torch.linspace(0., 1., 11, device=dev)[1:-1].contiguous()
        for est in (False, True):
            case(f"packed stage {P}x~{mean} m=9 estimate={int(est)}", lambda: _neus_upsample.upsample_stage_packed(d, sdf, pi, u, 64.0, est),
                 pick=lambda out: (out[0], out[1], out[3], out[4]))          # sdf_merged has places left for the caller
        case(f"packed stage {P}x~{mean} m=9 no merge", lambda: _neus_upsample.upsample_stage_packed(d, sdf, pi, u, 64.0, False, merge=False))
    for R, n in ((4096, 65), (4096, 260), (65536, 65), (65536, 260)):
        d = (0.5 + 3.0 * torch.rand(R, n, generator=gen)).sort(-1).values.contiguous().to(dev)
        sdf, u = (2.0 - d).contiguous(), torch.linspace(0., 1., 67, device=dev)[1:-1].contiguous()
        for est in (False, True):
            case(f"row stage {R}x({n}+65) estimate={int(est)}", lambda: _neus_upsample.upsample_stage(d, sdf, u, 64.0, est))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
