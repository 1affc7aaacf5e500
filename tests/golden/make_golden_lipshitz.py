#!/usr/bin/env python
"""tests/golden/make_golden_lipshitz.py -> tests/golden/ref_lipshitz_mlp.npz (data only, a few KB).

Recorded results of the reference's own ``nr3d_lib.models.blocks.mlp.LipshitzMLP`` in float32 on the CPU, two small networks:
    a: 5 -> 16 -> 16 -> 3, ReLU hidden layers, sigmoid output, c_init_factor 1.0
    b: 5 -> 16 -> 3, softplus(beta 100) hidden layer, no output activation, c_init_factor 2.0
For each: the state dict as constructed (``lipshitz_bound_per_layer`` = the initial bounds), an input of 7 rows, and for three states of the
bounds -- "init" (as constructed: softplus(c) > every row abs-sum, the normalisation is the identity), "half" (the bounds overwritten
with half their value, so that rows really are scaled; with c_init_factor 2.0 that is the inf-norm itself and still the identity) and
"quarter" (halved once more: rows of both networks are scaled) -- y, lipshitz_bound_full() and the gradients of y.sum() + lipshitz_bound_full()
with respect to x and every parameter.  Run from a checkout that has the reference next to it; the .npz is what the tests read."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

CASES = (
    ("a", dict(D=2, W=16, activation="relu", output_activation="sigmoid", c_init_factor=1.0)),
    ("b", dict(D=1, W=16, activation=dict(type="softplus", beta=100.0), output_activation=None, c_init_factor=2.0)),
)
IN, OUT, ROWS = 5, 3, 7
PHASES = ("init", "half", "quarter")       # the bounds as constructed, times 1/2, times 1/4


def main():
    mod = import_reference("nr3d_lib.models.blocks.mlp")
    out = {"cases": np.array([c[0] for c in CASES])}
    for k, (tag, cfg) in enumerate(CASES):
        torch.manual_seed(20261021 + k)
        m = mod.LipshitzMLP(IN, OUT, **cfg)
        x = torch.randn(ROWS, IN)
        out[f"{tag}_c_init_factor"] = np.float64(cfg["c_init_factor"])
        out[f"{tag}_x"] = x.numpy().copy()
        for name, val in m.state_dict().items():
            out[f"{tag}_sd_{name}"] = val.detach().numpy().copy()
        for phase in PHASES:
            if phase != "init":
                with torch.no_grad():
                    m.lipshitz_bound_per_layer.mul_(0.5)
            m.zero_grad(set_to_none=True)
            xr = x.clone().requires_grad_(True)
            y = m(xr)
            bound = m.lipshitz_bound_full()
            (y.sum() + bound).backward()
            out[f"{tag}_{phase}_y"] = y.detach().numpy().copy()
            out[f"{tag}_{phase}_bound"] = bound.detach().numpy().copy()
            out[f"{tag}_{phase}_gx"] = xr.grad.numpy().copy()
            for name, p in m.named_parameters():
                out[f"{tag}_{phase}_g_{name}"] = p.grad.numpy().copy()
        scaled = [float((l.weight.abs().sum(1) > torch.nn.functional.softplus(c)).float().mean())
                  for l, c in zip(m.layers, m.lipshitz_bound_per_layer)]
        print(f"case {tag}: fraction of scaled rows per layer at the last state {scaled}")
    path = os.path.join(HERE, "ref_lipshitz_mlp.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    main()
