#!/usr/bin/env python
"""tests/golden/make_golden_forest_ray_test.py -> tests/golden/ref_forest_ray_test.npz (data only, about 30 KB).

Recorded results of the reference's own slab test ``nr3d_lib.graphics.raytest.ray_box_intersection`` called the way its
``ForestBlockSpace.ray_test`` calls it (nr3d_lib/models/spatial/forest.py:356-363): every ray against every block box, float32 on the
CPU, ``t_min_cons`` = 0 / a number / a per-ray column, ``t_max_cons`` = None / a number / a per-ray column.  Per case the file holds
the forest (level, block coordinates in octree order, world origin and block size), the rays, the bounds and the reference's
``t_near``, ``t_far`` and ``mask`` [R, B].  Lattice rays (faces, edges, corners, zero direction components) and random ones.  Run from
a checkout that has the reference next to it; the .npz is what the tests read."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import forest_ray_test_ref as R  # noqa: E402
from make_golden import import_reference  # noqa: E402


def main():
    mod = import_reference("nr3d_lib.graphics.raytest")
    rng = np.random.default_rng(20261021)
    forests = {"plus": R.Forest(R.PLUS[1], R.PLUS[0], (-2.0, -2.0, -2.0), (1.0, 1.0, 1.0)),
               "l2_half": R.Forest(R.random_blocks(rng, 2, 0.5), 2, (0.3, -1.7, 2.9), (0.7, 0.35, 1.4))}
    out = {"cases": []}
    for name, fo in forests.items():
        o = np.concatenate([R.rays(fo, rng, 32, "lattice")[0], R.rays(fo, rng, 16, "random")[0]])
        d = np.concatenate([R.rays(fo, rng, 32, "lattice")[1], R.rays(fo, rng, 16, "random")[1]])
        n = o.shape[0]
        span = float((fo.world_block_size * (1 << fo.level)).max())
        bounds = {"none": (None, None), "number": (0.05, 0.6 * span),
                  "tensor": (rng.uniform(0.0, 0.3, n).astype(np.float32), rng.uniform(0.2 * span, 1.5 * span, n).astype(np.float32))}
        wb, wo = torch.from_numpy(fo.world_block_size), torch.from_numpy(fo.world_origin)
        bmin = torch.from_numpy(fo.block_ks.astype(np.float32)) * wb + wo
        for bname, (near, far) in bounds.items():
            col = lambda v: torch.from_numpy(v).unsqueeze(-1) if isinstance(v, np.ndarray) else v      # noqa: E731
            t_near, t_far, mask = mod.ray_box_intersection(
                torch.from_numpy(o).unsqueeze(1), torch.from_numpy(d).unsqueeze(1), aabb_min=bmin.unsqueeze(0),
                aabb_max=(bmin + wb).unsqueeze(0), t_min_cons=0. if near is None else col(near), t_max_cons=col(far))
            k = f"{name}_{bname}_"
            out["cases"].append(k[:-1])
            out[k + "level"], out[k + "block_ks"] = np.int64(fo.level), fo.block_ks
            out[k + "world_origin"], out[k + "world_block_size"] = fo.world_origin, fo.world_block_size
            out[k + "rays_o"], out[k + "rays_d"] = o, d
            out[k + "near"] = np.float32(0) if near is None else np.asarray(near, np.float32)
            out[k + "far"] = np.float32(np.inf) if far is None else np.asarray(far, np.float32)
            out[k + "t_near"], out[k + "t_far"], out[k + "mask"] = t_near.numpy(), t_far.numpy(), mask.numpy()
    out["cases"] = np.array(out["cases"])
    path = os.path.join(HERE, "ref_forest_ray_test.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out['cases'])} cases, {int(sum(out[c + '_mask'].sum() for c in out['cases']))} hits")


if __name__ == "__main__":
    main()
