#!/usr/bin/env python
"""Regenerates tests/golden/ref_neus_coarse.npz.  BUILD container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_neus_coarse.py

Outputs of the reference's own batched NeuS helpers (graphics/neus/neus_utils.py: neus_ray_sdf_to_upsample_alpha, neus_ray_sdf_to_tau,
neus_ray_sdf_to_vw, neus_estimate_sdf_nablas_to_alpha; graphics/raysample.py: batch_sample_pdf, batch_sample_cdf) on fixed inputs, and
of the reference's neus_ray_query_coarse_multi_upsample itself (graphics/neus/neus_ray_query.py:132-356) on the CPU: the analytic
sphere and ray fan of tests/neus_coarse_ref.py, compression=False, upsample_mode='multistep_estimate', num_coarse=16, num_fine=8,
both upsample_use_estimate_alpha values; `t` and `opacity_alpha` are kept.  Data only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import numpy as np
import torch

from make_golden import import_reference   # noqa: E402
from neus_coarse_ref import SphereModel, fan_rays   # noqa: E402

QUERY = dict(compression=False, upsample_mode='multistep_estimate', num_coarse=16, num_fine=8)


def main():
    nu = import_reference("nr3d_lib.graphics.neus.neus_utils")
    rs = import_reference("nr3d_lib.graphics.raysample")
    rq = import_reference("nr3d_lib.graphics.neus.neus_ray_query")
    out = {}
    torch.manual_seed(23)
    depth = torch.linspace(0.5, 3.0, 13).expand(5, 13) + 0.05 * torch.rand(5, 13)
    sdf = 1.2 - depth + 0.05 * torch.randn(5, 13)
    out.update(h_depth=depth, h_sdf=sdf, h_inv_s=np.float32(24.0))
    out["upsample_alpha"] = nu.neus_ray_sdf_to_upsample_alpha(sdf, depth, 24.0)
    out["tau"] = nu.neus_ray_sdf_to_tau(sdf, 24.0)
    out["tau_append"] = nu.neus_ray_sdf_to_tau(sdf, 24.0, append_cdf_1=True)
    out["vw"] = nu.neus_ray_sdf_to_vw(sdf, 24.0)
    nablas = torch.randn(5, 13, 3)
    dirs = torch.nn.functional.normalize(torch.randn(5, 1, 3), dim=-1).expand(5, 13, 3).contiguous()
    deltas = torch.rand(5, 13) * 0.2
    out.update(h_nablas=nablas, h_dirs=dirs, h_deltas=deltas)
    for ratio in (1, 0, 0.3):
        out[f"estimate_alpha_{ratio}"] = nu.neus_estimate_sdf_nablas_to_alpha(sdf, deltas.clone(), nablas, dirs, 24.0, ratio=ratio)
    weights = torch.rand(5, 12) ** 3
    weights[3] = 0                                  # a row without any weight
    out["h_weights"] = weights
    out["sample_pdf"] = rs.batch_sample_pdf(depth, weights, 7)
    cdf = torch.cat([torch.zeros(5, 1), torch.cumsum(weights / weights.sum(-1, keepdim=True).clamp_min(1e-5), -1)], -1)
    out["h_cdf"] = cdf
    out["sample_cdf"] = rs.batch_sample_cdf(depth, cdf, 7)

    rays = fan_rays()
    for est in (False, True):
        vb, _ = rq.neus_ray_query_coarse_multi_upsample(SphereModel(), rays, upsample_use_estimate_alpha=est, **QUERY)
        assert vb['type'] == 'batched' and tuple(vb['t'].shape) == (64, 52), vb['t'].shape
        out[f"query_t_est{int(est)}"] = vb['t']
        out[f"query_alpha_est{int(est)}"] = vb['opacity_alpha']
    out = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    path = os.path.join(HERE, "ref_neus_coarse.npz")
    np.savez_compressed(path, **out)
    print({k: getattr(v, "shape", v) for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
