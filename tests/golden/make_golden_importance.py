#!/usr/bin/env python
"""tests/golden/make_golden_importance.py -> tests/golden/ref_importance.npz: what the reference's own ErrorMap / ImpSampler
(nr3d_lib/models/importance.py) return on the CPU, data only.  ``scenario(mod)`` is the recorded sequence of calls on a module that
has the two classes; this script runs it on the reference, tests/test_importance_cpu.py runs it on the package and compares every array.

    python tests/golden/make_golden_importance.py      # needs the reference checkout (make_golden.import_reference)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_importance.npz")

SHAPES = [(3, 5, 7), (2, 3, 130), (4, 65, 9)]
CDF_CONFIGS = {"min01": dict(min_pdf=0.01), "min0": dict(min_pdf=0.0), "max": dict(min_pdf=0.01, max_pdf=0.7)}
SEED = 20240607
N_STEPS = 600


def update_inputs(N, H, W):
    """the recorded updates of one shape: {name: (i, xy, val)}; no two (sample, corner) pairs of one update share a cell"""
    g = torch.Generator().manual_seed(SEED + N * 1000 + H * 10 + W)
    scalar_xy = torch.tensor([[0.0, 0.0], [1.0, 1.0], [3.0 / W, 0.0 / H]], dtype=torch.float32)            # the last: a cell corner
    frames_xy = torch.tensor([[0.999, 0.5], [0.0, 0.0], [1.0, 1.0], [0.3, 0.3], [4.0 / W, 1.0 / H]], dtype=torch.float32)
    frames_i = torch.tensor([N - 1, 0, 0, N - 1, 1 % N], dtype=torch.long)
    return {"scalar": (N - 1, scalar_xy, torch.rand(scalar_xy.shape[0], generator=g)),
            "frames": (frames_i, frames_xy, torch.rand(frames_xy.shape[0], generator=g))}


def fresh_map(mod, N, H, W, **kw):
    m = mod.ErrorMap(N, (H, W), **kw)
    g = torch.Generator().manual_seed(SEED + N + H + W)
    m.error_map.copy_(torch.empty(N, H, W).uniform_(0.2, 1, generator=g))
    return m


def scenario(mod):
    """{name: numpy array}: every recorded result, in a fixed order of calls and seeds"""
    out = {}
    for (N, H, W) in SHAPES:
        tag = f"{N}x{H}x{W}"
        # updates, each on a fresh map
        for name, (i, xy, val) in update_inputs(N, H, W).items():
            m = fresh_map(mod, N, H, W)
            out[f"{tag}/map0"] = m.error_map.numpy().copy()
            m.update_error_map(i, xy, val)
            changed = np.flatnonzero(m.error_map.numpy() != out[f"{tag}/map0"])      # the cells the update wrote: where and what
            out[f"{tag}/update_{name}_cells"] = changed
            out[f"{tag}/update_{name}_values"] = m.error_map.numpy().reshape(-1)[changed].copy()
        # CDFs
        for cname, kw in CDF_CONFIGS.items():
            m = fresh_map(mod, N, H, W, **kw)
            m.construct_cdf()
            if "max_pdf" in kw:
                out[f"{tag}/{cname}/map_after"] = m.error_map.numpy().copy()
            else:
                out[f"{tag}/{cname}/map_unchanged"] = np.array([int(np.array_equal(m.error_map.numpy(), out[f"{tag}/map0"]))])
            for a in ("cdf_x_cond_y", "cdf_y", "cdf_img"):
                out[f"{tag}/{cname}/{a}"] = getattr(m, a).numpy().copy()
            m2 = fresh_map(mod, N, H, W, **kw)
            m2.construct_cdf_and_clean_error_map()
            out[f"{tag}/{cname}/clean_equal"] = np.array([int(all(torch.equal(getattr(m, a), getattr(m2, a))
                                                                  for a in ("cdf_x_cond_y", "cdf_y", "cdf_img"))),
                                                          int(bool((m2.error_map == 0).all()))])
        # sampling from a recorded seed
        m = fresh_map(mod, N, H, W)
        m.construct_cdf()
        torch.manual_seed(SEED)
        out[f"{tag}/sample_pixel_int"] = m.sample_pixel(64, N - 1).numpy().copy()
        frames = torch.randint(N, [64], dtype=torch.long)
        out[f"{tag}/sample_pixel_frames_in"] = frames.numpy().copy()
        out[f"{tag}/sample_pixel_frames"] = m.sample_pixel(64, frames).numpy().copy()
        out[f"{tag}/sample_img"] = m.sample_img(64).numpy().copy()
        i, xy = m.sample_img_pixel(64)
        out[f"{tag}/sample_img_pixel_i"], out[f"{tag}/sample_img_pixel_xy"] = i.numpy().copy(), xy.numpy().copy()
        out[f"{tag}/pdf_image"] = m.get_pdf_image().numpy().copy()
        if (N, H, W) == SHAPES[0]:
            out[f"{tag}/normalized"] = m.get_normalized_error_map().numpy().copy()
            out[f"{tag}/normalized_frame"] = m.get_normalized_error_map(1).numpy().copy()
    # an ImpSampler of two maps
    N = 3
    a, b = fresh_map(mod, N, 5, 7), fresh_map(mod, N, 9, 4, min_pdf=0.0)
    sampler = mod.ImpSampler({"a": (a, 0.3), "b": (b, 0.2)}, frac_uniform=0.5)
    out["imp/fracs"] = np.array(sampler.error_map_fracs)
    out["imp/pdf_image"] = sampler.get_pdf_image().numpy().copy()
    torch.manual_seed(SEED + 1)
    for n in (13, 1000):
        i, xy = sampler.sample_img_pixel(n)
        out[f"imp/{n}/i"], out[f"imp/{n}/xy"] = i.numpy().copy(), xy.numpy().copy()
        out[f"imp/{n}/sample_img"] = sampler.sample_img(n).numpy().copy()
        out[f"imp/{n}/sample_pixel"] = sampler.sample_pixel(n, 1).numpy().copy()
    for k, v in sampler.state_dict().items():
        out[f"imp/state_dict/{k}"] = v.numpy().copy()
    for k, v in a.state_dict().items():
        out[f"errmap/state_dict/{k}"] = v.numpy().copy()
    # the period schedule of step_error_map
    for name, n_max in (("max", 50), ("nomax", None)):
        m = mod.ErrorMap(2, (4, 4), n_steps_init=8, n_steps_max=n_max)
        g = torch.Generator().manual_seed(SEED + 2)
        sched = np.zeros((N_STEPS, 2), np.int64)
        for s in range(N_STEPS):
            m.step_error_map(s % 2, torch.rand(3, 2, generator=g), torch.rand(3, generator=g))
            sched[s] = (m.n_steps_between_update, m.n_steps_since_update)
        out[f"schedule/{name}"] = sched
    return out


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import importance_ref as ref
    from make_golden import import_reference
    mod = import_reference("nr3d_lib.models.importance")
    for (N, H, W) in SHAPES:
        for name, (i, xy, val) in update_inputs(N, H, W).items():
            # the reference's update keeps one of two contributions to a cell: undefined, so nothing of that kind is recorded
            assert not ref.cells_touched_twice(i if isinstance(i, int) else i.numpy(), xy.numpy(), val.numpy(), N, H, W), (N, H, W, name)
    out = scenario(mod)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
