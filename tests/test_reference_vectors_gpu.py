"""GPU: the HIP path against vectors produced by the REFERENCE's own Python code (tests/golden/ref_*.npz, generated in the
build container by tests/golden/make_golden*.py), directly -- not through the oracle.

  * BASELINE configs[0] (Dense 32^3 x 4 features, 65 536 points, forward) and a 2-D Dense level against the reference's
    pure-PyTorch sampler `param_interpolate` (lotd_helpers.py:274-346).  grid_sample's own coordinate arithmetic limits
    the agreement to ~1e-5 absolute on N(0, 1) parameters, hence 3e-5 here -- the same bound the
    oracle is held to against this fixture (tests/test_oracle_golden_cpu.py);
  * VM and CP levels against the reference's 1-D / 2-D samplers applied to every line / plane table it slices out of
    the flat parameter vector (what its rescale_volume does, lotd_encoding.py:350-402), combined with the level's
    definition (VM = sum_d plane_d * line_d, CP = prod_d line_d)."""
import os

import numpy as np
import pytest
import torch

from util import load_golden_param_interpolate

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("tag,D", [("c1", 3), ("d2", 2)])
def test_dense_forward_against_reference_param_interpolate(dev, tag, D):
    from nr3d_lib_amd.bindings import _lotd
    z = load_golden_param_interpolate()
    R, F = int(z[f"{tag}_res"]), int(z[f"{tag}_feats"])
    x, p, want = z[f"{tag}_x"], z[f"{tag}_params"].astype(np.float32), z[f"{tag}_y"]
    if tag == "c1":            # configs[0] exactly as BASELINE.json states it: Dense 32^3 x 4, all 65 536 points
        assert (R, F) == (32, 4) and p.size == 32 ** 3 * 4 and x.shape[0] == 65536
    m = _lotd.LoDMeta(D, [R], [F], ["Dense"], None)
    xt, pt = torch.from_numpy(x).to(dev), torch.from_numpy(p).to(dev)
    y, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
    got = y.cpu().numpy()
    assert got.shape == want.shape
    scale = np.abs(want).max(0)                                    # per output column
    assert (np.abs(got - want).max(0) <= 3e-5 * scale).all()
    # the Jacobian of the same call, against central differences of the reference's values is not available (the fixture
    # holds values only); consistency with the kernel's own forward: finite differences in fp64-promoted inputs
    h = 1e-3
    for d in range(D):
        e = np.zeros(D, np.float32); e[d] = h
        lo = np.floor(x.astype(np.float64) * (R - 2) + 0.5)
        keep = (np.floor((x + e).astype(np.float64) * (R - 2) + 0.5) == lo).all(1) & \
               (np.floor((x - e).astype(np.float64) * (R - 2) + 0.5) == lo).all(1) & ((x + e) < 1).all(1) & ((x - e) > 0).all(1)
        yp = _lotd.lod_fwd(m, torch.from_numpy(x + e).to(dev), pt)[0].cpu().numpy().astype(np.float64)
        ym = _lotd.lod_fwd(m, torch.from_numpy(x - e).to(dev), pt)[0].cpu().numpy().astype(np.float64)
        step = ((x + e)[:, d].astype(np.float64) - (x - e)[:, d].astype(np.float64))[:, None]
        fd = (yp - ym) / step
        jd = j.reshape(x.shape[0], F, D)[:, :, d].cpu().numpy()
        # inside a cell the interpolant is linear along d, so the central difference is exact up to fp32 rounding of y
        assert np.abs(fd - jd)[keep].max() <= 2e-3 * np.abs(jd).max()


@pytest.mark.parametrize("name,tp", [("vm", "VM"), ("cp", "CP")])
def test_vm_cp_forward_against_reference_table_samplers(dev, name, tp):
    from nr3d_lib_amd.bindings import _lotd
    z = np.load(os.path.join(GOLD, "ref_table_interpolate.npz"))
    R, F, x = int(z["res"]), int(z["feats"]), z["x"]
    m = _lotd.LoDMeta(3, [R], [F], [tp], None)
    y = _lotd.lod_fwd(m, torch.from_numpy(x).to(dev), torch.from_numpy(z[f"{name}_params"]).to(dev))[0].cpu().numpy()
    lines = [z[f"{name}_line{d}"].astype(np.float64) for d in range(3)]
    want = sum(z[f"vm_plane{d}"].astype(np.float64) * lines[d] for d in range(3)) if tp == "VM" else lines[0] * lines[1] * lines[2]
    assert y.shape == want.shape
    assert (np.abs(y - want).max(0) <= 5e-5 * np.abs(want).max(0)).all()
