#!/usr/bin/env python
"""Regenerates tests/golden/mlp_plan_sizes.npz: the four size queries of the fused decoder (nr3d_mlp_packed_floats,
nr3d_mlp_backward_packed_floats, nr3d_mlp_half_packed_bytes, nr3d_mlp_half_backward_packed_bytes) over a grid of networks, as the
library answers them.  No GPU and no reference needed: the queries are host arithmetic (csrc/mlp_plan.h and its users).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mlp_sizes.py [path/to/libnr3d_hip.so]

The fixture pins what the library computed BEFORE a change to that host code: write it from a build of the commit in front of the
change (the committed file comes from the last commit that had the plan copied into mlp.hip and mlp_half.hip), never from the
code under test.  tests/test_mlp_cpu.py::test_size_queries_match_the_recorded_plan compares with exact equality."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_LAYERS = 8
WIDTHS = (1, 32, 33, 64, 65, 96, 97, 128)
MIXED = ([32, 64, 32, 16], [32, 32, 64, 16], [18, 64, 33, 64, 3], [64, 32, 64, 64], [32, 16, 8, 4, 2, 1], [32, 128, 64, 16],
         [128, 64, 32, 64, 128], [3, 65, 64, 1], [32, 33, 32, 32, 16])
QUERIES = ("nr3d_mlp_packed_floats", "nr3d_mlp_backward_packed_floats", "nr3d_mlp_half_packed_bytes",
           "nr3d_mlp_half_backward_packed_bytes")


class CDesc(C.Structure):
    _fields_ = [("n_layers", C.c_uint32), ("dims", C.c_uint32 * (MAX_LAYERS + 1)), ("hidden_activation", C.c_uint32),
                ("output_activation", C.c_uint32)]


def networks():
    """every dims list of the grid: 2..8 linear layers x input, uniform hidden and output width; mixed hidden widths; the invalid
    widths 0 and 129 in each position"""
    nets = [[i] + [w] * (n - 1) + [o] for n in range(2, MAX_LAYERS + 1) for i, w, o in itertools.product(WIDTHS, repeat=3)]
    nets += [list(m) for m in MIXED]
    for bad in (0, 129):
        nets += [[bad, 64, 16], [32, bad, 16], [32, 64, bad], [32, 64, bad, 64, 16]]
    return nets


def query(lib, nets):
    out = np.zeros((len(nets), len(QUERIES)), np.uint64)
    for q in QUERIES:
        getattr(lib, q).restype, getattr(lib, q).argtypes = C.c_uint64, [C.c_void_p]
    for k, dims in enumerate(nets):
        c = CDesc()
        c.n_layers = len(dims) - 1
        for i, d in enumerate(dims):
            c.dims[i] = d
        c.hidden_activation, c.output_activation = 1, 0
        out[k] = [getattr(lib, q)(C.byref(c)) for q in QUERIES]
    return out


def pad(nets):
    a = np.zeros((len(nets), MAX_LAYERS + 2), np.uint32)               # [n_layers, dims...]
    for k, dims in enumerate(nets):
        a[k, 0] = len(dims) - 1
        a[k, 1:1 + len(dims)] = dims
    return a


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "..", "nr3d_lib_amd", "libnr3d_hip.so")
    nets = networks()
    sizes = query(C.CDLL(os.path.abspath(path)), nets)
    np.savez_compressed(os.path.join(HERE, "mlp_plan_sizes.npz"), nets=pad(nets), sizes=sizes, queries=np.array(QUERIES))
    print("wrote", len(nets), "networks,", int((sizes != 0).sum()), "non-zero sizes")


if __name__ == "__main__":
    main()
