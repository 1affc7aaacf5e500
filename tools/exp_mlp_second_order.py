#!/usr/bin/env python
"""tools/exp_mlp_second_order.py -- the SDF step's decoder half (LoTDSDF.forward_sdf_nablas): forward, create_graph first backward
(nablas) and the eikonal loss's backward through them, per route, alternated in one process:
  fused2: FUSED_SECOND_ORDER = True (k_mlp_bwd2), fused1: FUSED_SECOND_ORDER = False (torch double backward of the layer-by-layer
  evaluation), torch: USE_FUSED = False.  fp32 and half blocks; then the whole step with a 16-level LoTDEncoding in front.
    python tools/exp_mlp_second_order.py [--reps R] [--out FILE.json] [--quick] [--softplus BETA] [--parent-lib FILE.so]
--softplus BETA: the same three routes on softplus hidden layers (nn.Softplus(BETA): the reference's SDF decoders have 100) -- fused2 then
  also sets FUSED_SOFTPLUS_SECOND_ORDER (k_mlp_bwd2_sp) -- on 35->64->1 and 32->64->64->1 at 2^18 and 2^22 samples.
--parent-lib FILE.so (a libnr3d_hip.so built from the parent commit): the ReLU twins of those shapes at the C ABI, first backward and
  double backward, this build's library against the parent's, alternated in the same process -- the ReLU kernels must not have moved.
Milliseconds per part: median over R alternated rounds of (3 timed repetitions after one warm-up)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nr3d_lib_amd.models.blocks import MLP
from nr3d_lib_amd.models.blocks import mlp as mlp_mod

ROUTES = ("fused2", "fused1", "torch")
SHAPES = ([35, 64, 1], [32, 64, 64, 1], [32, 64, 64, 16], [64, 64, 64, 64])
SOFTPLUS_SHAPES = ([35, 64, 1], [32, 64, 64, 1])
SOFTPLUS_DEFAULT = mlp_mod.FUSED_SOFTPLUS_SECOND_ORDER


def set_route(r, softplus=False):
    mlp_mod.USE_FUSED = r != "torch"
    mlp_mod.FUSED_SECOND_ORDER = r == "fused2"
    mlp_mod.FUSED_SOFTPLUS_SECOND_ORDER = (r == "fused2") if softplus else SOFTPLUS_DEFAULT


def relu_twins(parent_path, n, reps, dev):
    """first backward and double backward of the ReLU twins through the C ABI, this library against the parent commit's"""
    from nr3d_lib_amd import _hip as H
    from nr3d_lib_amd.bindings import _mlp
    parent = C.CDLL(os.path.abspath(parent_path))
    try:
        H._declare(parent)
    except RuntimeError:
        pass                                      # entry points this build adds: not called below
    rows = []
    for dims in SOFTPLUS_SHAPES:
        torch.manual_seed(0)
        m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation="relu", dtype=torch.float, device=dev)
        desc = m.fused_desc()
        ws, bs = [l.weight for l in m.layers], [l.bias for l in m.layers]
        x, v = torch.randn(n, dims[0], device=dev), torch.randn(n, dims[0], device=dev)
        gy = torch.ones(n, dims[-1], device=dev)
        packed = _mlp.pack(desc, ws, bs, with_backward=True)
        dx, dgy = torch.empty_like(x), torch.empty_like(gy)
        st = H.stream_of(x)

        def parts(lib):
            def check(rc):
                if rc != 0:
                    raise RuntimeError(lib.nr3d_last_error().decode())

            def backward():
                dWs, dbs = _mlp._grad_pool(desc, [True] * len(ws), dev)
                check(lib.nr3d_mlp_backward(C.byref(desc._c), n, H.ptr(x), dims[0], 1, H.ptr(gy), dims[-1], H.ptr(packed), H.ptr(dx), dims[0], 1,
                                            _mlp._ptr_array(dWs), _mlp._ptr_array(dbs), st))

            def backward_backward():
                dWs, _ = _mlp._grad_pool(desc, [False] * len(ws), dev)
                check(lib.nr3d_mlp_backward_backward(C.byref(desc._c), n, H.ptr(x), dims[0], 1, H.ptr(gy), dims[-1], H.ptr(v), dims[0], 1,
                                                     H.ptr(packed), H.ptr(dgy), dims[-1], _mlp._ptr_array(dWs), st))
            return dict(backward=backward, backward_backward=backward_backward)
        routes = {"this": parts(H.lib()), "parent": parts(parent)}
        res = {r: {k: [] for k in p} for r, p in routes.items()}
        for rnd in range(reps):
            for r in (list(routes)[::-1] if rnd & 1 else list(routes)):      # alternated, odd rounds in reverse order
                for k, fn in routes[r].items():
                    fn()
                    torch.cuda.synchronize()
                    a, b = ev(), None
                    for _ in range(3):
                        fn()
                    b = ev()
                    torch.cuda.synchronize()
                    res[r][k].append(a.elapsed_time(b) / 3)
        ms = {r: {k: round(median(t), 4) for k, t in d.items()} for r, d in res.items()}
        row = dict(what="ReLU at the C ABI, this library against the parent commit's", dims=dims, n=n, ms=ms,
                   this_over_parent={k: round(ms["this"][k] / ms["parent"][k], 4) for k in ms["this"]})
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def timed(fn, reps=3):
    """ms per call of fn, which returns the events of its parts: [(name, start, end)]"""
    fn()
    torch.cuda.synchronize()
    acc = {}
    for _ in range(reps):
        parts = fn()
        torch.cuda.synchronize()
        for name, a, b in parts:
            acc[name] = acc.get(name, 0.0) + a.elapsed_time(b) / reps
    return acc


def ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def decoder_step(m, x0):
    def run():
        m.zero_grad(set_to_none=True)
        x = x0.detach().requires_grad_(True)
        e0 = ev()
        y = m(x)
        e1 = ev()
        nablas, = torch.autograd.grad(y[:, 0].float().sum(), x, create_graph=True)
        e2 = ev()
        loss = ((nablas.float().norm(dim=-1) - 1.0) ** 2).mean() + y[:, 0].float().abs().mean()
        e3 = ev()
        loss.backward()
        e4 = ev()
        return [("forward", e0, e1), ("grad_create_graph", e1, e2), ("eikonal_backward", e3, e4), ("step", e0, e4)]
    return run


def sdf_step(enc, dec, x0):
    def run():
        enc.zero_grad(set_to_none=True)
        dec.zero_grad(set_to_none=True)
        x = x0.detach().requires_grad_(True)
        e0 = ev()
        h, dy_dx = enc.forward_dydx(x)
        h_in = torch.cat([h, x], dim=-1)
        sdf = dec(h_in)[..., 0]
        dL_dh, = torch.autograd.grad(sdf, h_in, torch.ones_like(sdf), create_graph=True)
        nablas = enc.backward_dydx(dL_dh[..., :32].contiguous(), dy_dx, x) + dL_dh[..., 32:]
        loss = ((nablas.norm(dim=-1) - 1.0) ** 2).mean() + sdf.abs().mean()
        loss.backward()
        e1 = ev()
        return [("step", e0, e1)]
    return run


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="2^16 samples only (a smoke run of the tool)")
    ap.add_argument("--softplus", type=float, default=None, metavar="BETA", help="softplus hidden layers with this beta")
    ap.add_argument("--parent-lib", default=None, help="libnr3d_hip.so of the parent commit: the ReLU A/B")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sp = args.softplus is not None
    act = dict(type="softplus", beta=args.softplus) if sp else "relu"
    sizes = [1 << 16] if args.quick else [1 << 18, 1 << 22] if sp else [1 << 20, 1 << 22]
    rows = []
    for dims in (SOFTPLUS_SHAPES if sp else SHAPES):
        for dtype in (torch.float32, torch.float16):
            torch.manual_seed(0)
            m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation=act, dtype=dtype, device=dev)
            desc = m.fused_desc()
            for n in sizes:
                x0 = torch.randn(n, dims[0], device=dev)
                res = {r: {} for r in ROUTES}
                for _ in range(args.reps):
                    for r in ROUTES:                           # alternated: every round runs every route once
                        set_route(r, sp)
                        for k, v in timed(decoder_step(m, x0)).items():
                            res[r].setdefault(k, []).append(v)
                set_route("fused2")
                row = dict(dims=dims, dtype=str(dtype).replace("torch.", ""), n=n, activation=act,
                           second_order_fusable=bool(desc and (desc.softplus_second_order_fusable if sp else desc.second_order_fusable)),
                           ms={r: {k: round(median(v), 4) for k, v in res[r].items()} for r in ROUTES})
                rows.append(row)
                print(json.dumps(row), flush=True)
                del x0
            del m
            torch.cuda.empty_cache()
    # the SDF step end to end: 16-level LoTD (32 features) + MLP(35 -> 64 -> 1)
    from nr3d_lib_amd.models.grid_encodings.lotd import LoTDEncoding, gen_ngp_cfg
    cfg = gen_ngp_cfg(num_levels=16)
    torch.manual_seed(0)
    enc = LoTDEncoding(3, lotd_cfg=dict(lod_res=cfg["lod_res"], lod_n_feats=cfg["lod_n_feats"], lod_types=cfg["lod_types"],
                                        hashmap_size=cfg["hashmap_size"]), dtype=torch.float, device=dev)
    dec = MLP(35, 1, D=1, W=64, activation=act, dtype=torch.float, device=dev)
    for n in sizes:
        x0 = torch.rand(n, 3, device=dev) * 1.8 - 0.9
        res = {r: [] for r in ROUTES}
        for _ in range(args.reps):
            for r in ROUTES:
                set_route(r, sp)
                res[r].append(timed(sdf_step(enc, dec, x0))["step"])
        set_route("fused2")
        row = dict(sdf_step="LoTD16 + MLP(35->64->1)", n=n, activation=act, ms={r: round(median(v), 4) for r, v in res.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.parent_lib:
        rows += relu_twins(args.parent_lib, sizes[-1], args.reps, dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
