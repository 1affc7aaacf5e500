#!/usr/bin/env python
"""tools/exp_mlp_sigmoid.py -- the sigmoid output activation (the reference's radiance decoders) on the fused decoder kernels:
  1. MLP(32 -> 64 -> 64 -> 3, ReLU hidden, sigmoid output), fp32 and half blocks, forward alone (no_grad) and forward + first backward,
     route "fused" against route "torch" = USE_FUSED False, the layer-by-layer evaluation such a module ran before the kernels took
     sigmoid -- alternated in one process;
  2. the cost of the sigmoid itself: the same shape at the C ABI of this library, sigmoid output against no output activation;
  3. with --parent-lib (a libnr3d_hip.so built from the parent commit): the existing twins -- ReLU output and no output activation at
     32 -> 64 -> 64 -> 16 and 35 -> 64 -> 1 -- at the C ABI, this build's library against the parent's, alternated in the same process;
     and parent against parent (a second copy of the same file, loaded as a library of its own): the spread two runs of IDENTICAL code
     show on this box, which is the margin the this-against-parent ratios are read with.
    python tools/exp_mlp_sigmoid.py [--reps R] [--parent-lib FILE.so] [--out FILE.json] [--quick]
Milliseconds: median over R alternated rounds of (3 timed repetitions after one warm-up), 2^22 samples."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nr3d_lib_amd import _hip as H
from nr3d_lib_amd.bindings import _mlp
from nr3d_lib_amd.models.blocks import MLP
from nr3d_lib_amd.models.blocks import mlp as mlp_mod

RADIANCE = [32, 64, 64, 3]
TWINS = ([32, 64, 64, 16], [35, 64, 1])


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def module_parts(m, x0, gy):
    def forward():
        with torch.no_grad():
            m(x0)

    def forward_backward():
        m.zero_grad(set_to_none=True)
        x = x0.detach().requires_grad_(True)
        m(x).backward(gy)
    return dict(forward=forward, forward_backward=forward_backward)


def abi_parts(lib, desc, ws, bs, x, gy, half):
    """forward / forward + backward of one library through the C ABI (the calls of bindings._mlp, with `lib` in H.lib()'s place)"""
    dt = torch.float16 if half else torch.float32
    n, dev = x.shape[0], x.device
    pre = "nr3d_mlp_half_" if half else "nr3d_mlp_"
    nbytes = (desc.half_packed_bytes + desc.half_backward_bytes) if half else 4 * (desc.packed_floats + desc.backward_floats)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    wh, bh = [w.detach().to(dt).contiguous() for w in ws], [b.detach().to(dt).contiguous() for b in bs]
    y = torch.empty(n, desc.dims[-1], dtype=dt, device=dev)
    dx = torch.empty(n, desc.dims[0], dtype=dt, device=dev)
    st = H.stream_of(x)

    def check(rc):
        if rc != 0:
            raise RuntimeError(lib.nr3d_last_error().decode())

    def forward():
        check(getattr(lib, pre + "pack")(C.byref(desc._c), _mlp._ptr_array(wh), _mlp._ptr_array(bh), H.ptr(packed), 1, st))
        check(getattr(lib, pre + "forward")(C.byref(desc._c), n, H.ptr(x), x.shape[1], 1, H.ptr(packed), H.ptr(y), y.shape[1], st))

    def forward_backward():
        forward()
        dWs, dbs = _mlp._grad_pool(desc, [True] * len(ws), dev)
        check(getattr(lib, pre + "backward")(C.byref(desc._c), n, H.ptr(x), x.shape[1], 1, H.ptr(gy), gy.shape[1], H.ptr(packed), H.ptr(dx),
                                             dx.shape[1], 1, _mlp._ptr_array(dWs), _mlp._ptr_array(dbs), st))
    return dict(forward=forward, forward_backward=forward_backward)


def alternate(routes, reps):
    """routes: {name: {part: fn}} (with an optional "enter" hook per route) -> {name: {part: median ms}}"""
    res = {r: {} for r in routes}
    for rnd in range(reps):
        # alternated: every round runs every route once, odd rounds in reverse order (no route is always the one that runs first)
        for r, parts in (list(routes.items())[::-1] if rnd & 1 else routes.items()):
            parts.get("enter", lambda: None)()
            for k, fn in parts.items():
                if k != "enter":
                    res[r].setdefault(k, []).append(timed(fn))
    return {r: {k: round(median(v), 4) for k, v in d.items()} for r, d in res.items()}


def ratio(ms, a, b):
    return {k: round(ms[a][k] / ms[b][k], 4) for k in ms[a]}


def load_copy(path, tmp, name):
    """a library of its own from a copy of `path` (the loader hands back the same handle for the same file)"""
    dst = os.path.join(tmp, name)
    shutil.copyfile(path, dst)
    lib = C.CDLL(dst)
    H._declare(lib)
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libnr3d_hip.so of the parent commit: the A/B of the existing kernels")
    ap.add_argument("--quick", action="store_true", help="2^16 samples (a smoke run of the tool)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 1 << 16 if args.quick else 1 << 22
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def net(dims, out=None):
        torch.manual_seed(0)
        m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation="relu", output_activation=out, dtype=torch.float, device=dev)
        return m, [l.weight for l in m.layers], [l.bias for l in m.layers]

    # 1. the radiance decoder as a module: fused against layer by layer
    dims = RADIANCE
    for dtype in (torch.float32, torch.float16):
        torch.manual_seed(0)
        m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation="relu", output_activation="sigmoid", dtype=dtype, device=dev)
        desc = m.fused_desc()
        assert desc is not None and desc.output_activation == _mlp.ACT_SIGMOID
        assert desc.half_backward_fusable if dtype == torch.float16 else desc.backward_fusable
        x0 = torch.randn(n, dims[0], device=dev)
        gy = torch.randn(n, dims[-1], device=dev).to(dtype)
        parts = module_parts(m, x0, gy)
        ms = alternate({"fused": dict(enter=lambda: setattr(mlp_mod, "USE_FUSED", True), **parts),
                        "torch": dict(enter=lambda: setattr(mlp_mod, "USE_FUSED", False), **parts)}, args.reps)
        mlp_mod.USE_FUSED = True
        emit(dict(what="sigmoid output, fused kernels against the layer-by-layer route", dims=dims, dtype=str(dtype).replace("torch.", ""),
                  n=n, ms=ms, torch_over_fused=ratio(ms, "torch", "fused")))
        del m, x0, gy
        torch.cuda.empty_cache()

    # 2. what the sigmoid itself costs: the same shape on this library, sigmoid output against no output activation
    for half in (False, True):
        m, ws, bs = net(dims)
        dt = torch.float16 if half else torch.float32
        x = torch.randn(n, dims[0], device=dev).to(dt)
        gy = torch.randn(n, dims[-1], device=dev).to(dt)
        routes = {name: abi_parts(H.lib(), _mlp.MLPDesc(dims, _mlp.ACT_RELU, code), ws, bs, x, gy, half)
                  for name, code in (("sigmoid", _mlp.ACT_SIGMOID), ("none", _mlp.ACT_NONE))}
        ms = alternate(routes, args.reps)
        emit(dict(what="the sigmoid's own cost at the C ABI: sigmoid output against no output activation, this library", dims=dims,
                  dtype="float16" if half else "float32", n=n, ms=ms, sigmoid_over_none=ratio(ms, "sigmoid", "none")))
        del m, x, gy
        torch.cuda.empty_cache()

    # 3. the existing kernels: this library against the parent commit's, and the parent's against itself
    if args.parent_lib:
        with tempfile.TemporaryDirectory() as tmp:
            parent = load_copy(os.path.abspath(args.parent_lib), tmp, "parent_a.so")
            parent_b = load_copy(os.path.abspath(args.parent_lib), tmp, "parent_b.so")
            for dims in TWINS:
                for out_name, out_code in (("relu", _mlp.ACT_RELU), (None, _mlp.ACT_NONE)):
                    for half in (False, True):
                        m, ws, bs = net(dims, out_name)
                        desc = _mlp.MLPDesc(dims, _mlp.ACT_RELU, out_code)
                        dt = torch.float16 if half else torch.float32
                        x = torch.randn(n, dims[0], device=dev).to(dt)
                        gy = torch.randn(n, dims[-1], device=dev).to(dt)
                        ms = alternate({"this": abi_parts(H.lib(), desc, ws, bs, x, gy, half),
                                        "parent": abi_parts(parent, desc, ws, bs, x, gy, half),
                                        "parent_again": abi_parts(parent_b, desc, ws, bs, x, gy, half)}, args.reps)
                        emit(dict(what="existing kernels at the C ABI: this library against the parent commit's, and the parent's against itself",
                                  dims=dims, output=out_name or "none", dtype="float16" if half else "float32", n=n, ms=ms,
                                  this_over_parent=ratio(ms, "this", "parent"), parent_over_parent=ratio(ms, "parent_again", "parent")))
                        del m, x, gy
                        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
