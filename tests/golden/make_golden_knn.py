#!/usr/bin/env python
"""tests/golden/make_golden_knn.py -> tests/golden/ref_knn.npz (data only, a few KB).

Recorded results of the reference's own Python layer ``nr3d_lib.maths.pytorch3d_knn``: ``knn_points(..., return_nn=True)`` (its sort,
pad and ``knn_gather``) and the gradients autograd takes through its Function, float32 on the CPU.  Its compiled extension
``nr3d_lib.bindings._pytorch3d_knn`` does not exist here; the stub's ``knn_points_idx`` / ``knn_points_backward`` are pointed at
tests/knn_ref.py, so what the file pins is the reference WRAPPER's semantics on top of the contract's kernel results.  Inputs are lattice
inputs (exact in float32, full of ties) with ragged ``lengths1`` / ``lengths2``, ``lengths2 < K`` and a zero length among them;
``grad_dists`` are powers of two.  Run from a checkout that has the reference next to it; the .npz is what the tests read."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import knn_ref as R  # noqa: E402
from make_golden import import_reference  # noqa: E402

CASES = (("a", 3, 4, 2), ("b", 3, 1, 1), ("c", 2, 5, 2), ("d", 4, 3, 1))      # tag, D, K, norm
N, P1, P2 = 3, 7, 9
LENGTHS1, LENGTHS2 = (0, 5, 7), (2, 9, 0)


def main():
    mod = import_reference("nr3d_lib.maths.pytorch3d_knn")

    def knn_points_idx(p1, p2, lengths1, lengths2, norm, K, version):
        idx, dists = R.knn_points(p1.numpy(), p2.numpy(), lengths1.numpy(), lengths2.numpy(), norm, K)
        return torch.from_numpy(idx), torch.from_numpy(dists)

    def knn_points_backward(p1, p2, lengths1, lengths2, idx, norm, grad_dists):
        g1, g2 = R.knn_backward(p1.numpy(), p2.numpy(), lengths1.numpy(), lengths2.numpy(), idx.numpy(), norm, grad_dists.numpy())[:2]
        return torch.from_numpy(g1.astype(np.float32)), torch.from_numpy(g2.astype(np.float32))

    mod._C.knn_points_idx = knn_points_idx
    mod._C.knn_points_backward = knn_points_backward
    rng = np.random.default_rng(20261021)
    out = {"cases": np.array([c[0] for c in CASES]), "lengths1": np.array(LENGTHS1, np.int64), "lengths2": np.array(LENGTHS2, np.int64)}
    for tag, D, K, norm in CASES:
        p1 = torch.from_numpy(R.lattice(rng, (N, P1, D), kmax=4)).requires_grad_(True)
        p2 = torch.from_numpy(R.lattice(rng, (N, P2, D), kmax=4)).requires_grad_(True)
        g = torch.from_numpy((2.0 ** rng.integers(-2, 3, size=(N, P1, K))).astype(np.float32))
        res = mod.knn_points(p1, p2, torch.tensor(LENGTHS1), torch.tensor(LENGTHS2), norm=norm, K=K, return_nn=True)
        g1, g2 = torch.autograd.grad(res.dists, (p1, p2), g)
        want_idx, want_dists = R.knn_points(p1.detach().numpy(), p2.detach().numpy(), LENGTHS1, LENGTHS2, norm, K)
        assert np.array_equal(res.idx.numpy(), want_idx) and np.array_equal(res.dists.detach().numpy(), want_dists), tag
        k = f"{tag}_"
        out[k + "D"], out[k + "K"], out[k + "norm"] = np.int64(D), np.int64(K), np.int64(norm)
        out[k + "p1"], out[k + "p2"], out[k + "grad_dists"] = p1.detach().numpy(), p2.detach().numpy(), g.numpy()
        out[k + "dists"], out[k + "idx"], out[k + "knn"] = res.dists.detach().numpy(), res.idx.numpy(), res.knn.detach().numpy()
        out[k + "grad_p1"], out[k + "grad_p2"] = g1.numpy(), g2.numpy()
    path = os.path.join(HERE, "ref_knn.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    main()
