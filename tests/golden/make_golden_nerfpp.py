#!/usr/bin/env python
"""Regenerates tests/golden/ref_nerfpp_march.npz.  BUILD container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nerfpp.py

Outputs of the reference's own NeRFRendererMixinDistant._ray_marching (models/fields_distant/nerf/renderer_mixin.py:170-288) on the CPU:
the unbound method with a SimpleNamespace for `self` and the reference's AABBSpace; its first statement refuses CPU tensors, so rays_o
goes in as a tensor subclass that answers True to `is_cuda`.  perturb=False, include_inf_distance=True, radius_scale 1 .. 100, the 12
rays of tests/nerfpp_march_ref.py::golden_rays, four sample modes x three interval types x max_steps in (8, 33, 100).  Per case
`<mode>.<interval>.<max_steps>.<field>` for the six fields of the returned tuple (a case without a valid sample stores `.none`).
Data only."""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import numpy as np
import torch

from make_golden import import_reference   # noqa: E402
import nerfpp_march_ref as ref   # noqa: E402

STEPS = (8, 33, 100)
FIELDS = ("ridx_hit", "samples", "depth_samples", "deltas", "ridx", "pack_infos")


class _SaysCuda(torch.Tensor):
    is_cuda = property(lambda self: True)


def main():
    rm = import_reference("nr3d_lib.models.fields_distant.nerf.renderer_mixin")
    spatial = import_reference("nr3d_lib.models.spatial")
    aabb, o, d, t_min = ref.golden_rays()
    space = spatial.AABBSpace(aabb=aabb)
    me = types.SimpleNamespace(space=space, radius_scale_min=1.0, radius_scale_max=100.0, include_inf_distance=True)
    out = dict(aabb=aabb.numpy(), rays_o=o.numpy(), rays_d=d.numpy(), t_min=t_min.numpy())
    for mode in ref.MODES:
        for interval in ref.INTERVALS:
            for steps in STEPS:
                ret = rm.NeRFRendererMixinDistant._ray_marching(me, o.clone().as_subclass(_SaysCuda), d.clone(), t_min.clone(), None,
                                                                 perturb=False, max_steps=steps, sample_mode=mode, interval_type=interval)
                key = f"{mode}.{interval}.{steps}"
                if ret.ridx_hit is None:
                    out[key + ".none"] = np.zeros(0, np.float32)
                    continue
                for f in FIELDS:
                    v = getattr(ret, f).as_subclass(torch.Tensor).detach().numpy()
                    out[f"{key}.{f}"] = v.astype(np.float32) if v.dtype.kind == "f" else v.astype(np.int64)
                n = np.zeros(o.shape[0], np.int64)
                n[out[key + ".ridx_hit"]] = out[key + ".pack_infos"][:, 1]
                print(key, n.tolist(), "NaN deltas:", int(np.isnan(out[key + ".deltas"]).sum()))
    path = os.path.join(HERE, "ref_nerfpp_march.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
