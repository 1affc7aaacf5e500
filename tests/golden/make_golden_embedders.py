#!/usr/bin/env python
"""tests/golden/make_golden_embedders.py -> tests/golden/ref_embedders.npz (data only).

Recorded results of the reference's own host-side embedders on seeded inputs in [-1, 1], float32 on the CPU:
  * ``get_sinusoidal_embedder(n_freq, D)`` (``SinusoidalEmbedder``) for D in {1, 3, 4}, n_freq in {0, 1, 6, 10}: outputs y,
    n = autograd.grad(y, x, g, create_graph=True), and the gradients of mean((|n| - 1)^2) w.r.t. x and g (zeros where autograd has no
    path); key prefix ``sin_D{D}_n{n}_``;
  * ``c_ref``: the largest residual, in units of 2^-24, of those outputs against sin64(2^f x + k pi/2) after half an ulp32 of the
    argument is taken off -- what the reference's own fp32 sine costs on this machine's torch;
  * ``AnnealedSinusoidalEmbedder`` (D = 3, 6 bands) at alpha = 0, 0.45, 1; key prefix ``ann_``;
  * ``maths/spherical_harmonics.eval_sh`` with one-hot coefficients on unit directions, deg 4 (25 columns); ``sh_degrees``: the number
    of BANDS (a degree of SHEncoder) for which it spans the same basis as tests/embedders_ref.py, checked here.
Run from a checkout that has the reference next to it; the .npz is what the tests read."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import embedders_ref as R  # noqa: E402
from make_golden import import_reference  # noqa: E402

B = 32


def main():
    sp = import_reference("nr3d_lib.models.embedders.sinusoidal_pytorch")
    shm = import_reference("nr3d_lib.maths.spherical_harmonics")
    rng = np.random.default_rng(20261016)
    out = {}
    c_ref = 0.0
    for D in (1, 3, 4):
        for n in (0, 1, 6, 10):
            m, C = sp.get_sinusoidal_embedder(n, input_dim=D)
            x = torch.from_numpy(rng.uniform(-1, 1, (B, D)).astype(np.float32)).requires_grad_(True)
            g = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32)).requires_grad_(True)
            y = m(x)
            nab, = torch.autograd.grad(y, x, g, create_graph=True)
            loss = ((nab.norm(dim=-1) - 1) ** 2).mean()
            dx, dg = torch.autograd.grad(loss, (x, g), allow_unused=True)
            k = f"sin_D{D}_n{n}_"
            out[k + "x"], out[k + "g"], out[k + "y"] = x.detach().numpy(), g.detach().numpy(), y.detach().numpy()
            out[k + "nablas"] = nab.detach().numpy()
            out[k + "dx"] = np.zeros((B, D), np.float32) if dx is None else dx.numpy()
            out[k + "dg"] = np.zeros((B, C), np.float32) if dg is None else dg.numpy()
            if n:
                xs = out[k + "x"]
                res = np.abs(out[k + "y"].astype(np.float64) - R.freq_forward(xs, n)) - R.freq_arg_term(xs, n)
                c_ref = max(c_ref, float(res[:, D:].max()) / R.EPS)
    out["c_ref"] = np.float64(max(c_ref, 0.0))
    m, _ = sp.get_sinusoidal_embedder(6, input_dim=3, annealed=True)
    x = torch.from_numpy(rng.uniform(-1, 1, (B, 3)).astype(np.float32))
    out["ann_x"], out["ann_alphas"] = x.numpy(), np.array([0.0, 0.45, 1.0])
    for i, a in enumerate(out["ann_alphas"]):
        m.set_cosine_easing_window(float(a))
        out[f"ann_y{i}"] = m(x).numpy()
    d = rng.standard_normal((B, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    basis = shm.eval_sh(4, torch.eye(25).expand(B, 25, 25), torch.from_numpy(d)).numpy()
    want = R.sh(d, 5)
    ok = 0
    for l in range(5):
        if np.abs(basis[:, l * l:(l + 1) ** 2] - want[:, l * l:(l + 1) ** 2]).max() > 2e-6:
            break
        ok = l + 1
    out["sh_dirs"], out["sh_basis"], out["sh_degrees"] = d, basis[:, :ok * ok], np.int64(ok)
    path = os.path.join(HERE, "ref_embedders.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, c_ref = {out['c_ref']:.3f}, eval_sh spans the same basis for {ok} bands")


if __name__ == "__main__":
    main()
