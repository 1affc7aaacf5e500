"""The packed up-sampling stage of the NeuS occupancy-march queries without a GPU: the restatement the GPU tests measure the HIP
kernel against (tests/neus_packed_ref.py) anchored to the CPU oracle's pack ops, the ABI entries, and the preconditions of the GPU
parity cases asserted on their inputs.

Anchor.  Both sides get the same float32 opacities.  The oracle's chain is packed_alpha_to_vw_forward (serial product, as the
restatement's cumprod), an exclusive float32 cumsum divided by max(last, 1e-5), packed_invert_cdf and
try_merge_two_packs_sorted_aligned.  Weights, CDF and the bin found are the same float32 operations in the same order on both
sides; the lerp is one fma on both, the restatement's through a float64 product that is rounded twice, so `fine` may differ by one
ulp of the depth and nothing else may differ at all.

Preconditions.  The parity packs are uniform depths in [NEAR, FAR] on the rays of fan_rays(4).  Packs of one and two elements carry
no mass there (both ends lie outside the sphere) and are compared exactly; a pack of three has its middle sample inside the sphere,
carries all its mass in the first interval and is compared by tolerance like the longer ones.  The smallest transmittance margin
over the cases is 0.13 % (estimate formula, inv_s = 64, L = 512), printed per case."""
import numpy as np
import pytest
import torch

import neus_coarse_ref as cref
import neus_packed_ref as ref
from nr3d_lib_amd import _abi

LENGTHS = [1, 2, 3, 5, 17, 33, 63, 64, 65, 128, 129, 200, 503, 504, 1031]


@pytest.mark.parametrize("est", [False, True])
@pytest.mark.parametrize("inv_s", [64.0, 1024.0])
def test_restatement_matches_oracle_chain(oracle, est, inv_s):
    depth, sdf, pi = ref.sphere_packs(LENGTHS)
    m = 9
    u = cref.shared_u(m)
    r = ref.stage(depth, sdf, pi, u, inv_s, est, torch.float32)
    alpha, pinfo = r['alpha'].numpy(), pi.numpy()
    w = oracle.packed_alpha_to_vw_forward(alpha, pinfo, 1e-4, 0.0, False)[0]
    cdf = np.zeros_like(w)
    for b, n in pinfo:
        c = np.concatenate([[0], np.cumsum(w[b:b + n - 1], dtype=np.float32)]).astype(np.float32)
        cdf[b:b + n] = c / max(c[-1], np.float32(1e-5))
    fine = oracle.packed_invert_cdf(depth.numpy(), cdf, np.ascontiguousarray(np.broadcast_to(u.numpy(), (len(pinfo), m))), pinfo)[0]
    ulp = np.spacing(np.abs(fine).astype(np.float32))
    assert (np.abs(fine.astype(np.float64) - r['fine'].double().numpy()) <= ulp).all()
    # the union of the oracle's own new depths: positions and packs exactly
    lb = [torch.searchsorted(depth[b:b + n].contiguous(), torch.from_numpy(fine[p]).contiguous()) for p, (b, n) in enumerate(pinfo)]
    pinfo_fine = np.stack([np.arange(len(pinfo)) * m, np.full(len(pinfo), m)], 1).astype(np.int64)
    pa, pb, pim = oracle.try_merge_two_packs_sorted_aligned(depth.numpy(), pinfo, fine.ravel(), pinfo_fine, b_sorted=True)
    for p, (b, n) in enumerate(pinfo):
        start, old, new = ref.merge_positions(int(b), int(n), lb[p], p)
        assert (start, n + m) == tuple(pim[p])
        np.testing.assert_array_equal(pa[b:b + n], old.numpy())
        np.testing.assert_array_equal(pb[p * m:(p + 1) * m], new.numpy())
    if np.array_equal(fine, r['fine'].numpy()):       # (and then the restatement's own positions are the oracle's)
        np.testing.assert_array_equal(pa, r['pidx_old'].numpy())
        np.testing.assert_array_equal(pb.reshape(-1, m), r['pidx_fine'].numpy())
        np.testing.assert_array_equal(pim, r['pack_infos_out'].numpy())


def test_merge_puts_a_new_depth_before_an_equal_old_one(oracle):
    a = np.array([1, 2, 2, 3, 5, 5], np.float32)
    b = np.array([0.5, 2, 2, 5, 6, 6], np.float32)
    pa, pb, pim = oracle.try_merge_two_packs_sorted_aligned(a, np.array([[0, 6]]), b, np.array([[0, 6]]), b_sorted=True)
    lb = torch.searchsorted(torch.from_numpy(a), torch.from_numpy(b))
    start, old, new = ref.merge_positions(0, 6, lb, 0)
    np.testing.assert_array_equal(pa, old.numpy())
    np.testing.assert_array_equal(pb, new.numpy())
    assert new.tolist() == [0, 2, 3, 7, 10, 11] and old.tolist() == [1, 4, 5, 6, 8, 9]


def test_abi_lists_the_packed_stage():
    assert _abi.ABI_VERSION >= 18
    ret, args = _abi.SIGNATURES['nr3d_neus_upsample_stage_packed']
    assert ret == 'int' and args == ['uint32_t', 'uint64_t', 'uint32_t'] + ['ptr'] * 4 + ['int64_t', 'float', 'int', 'int', 'int'] \
        + ['ptr'] * 6 + ['ptr']
    assert _abi.SIGNATURES['nr3d_neus_upsample_packed_lds_row'] == ('int', [])


@pytest.mark.parametrize("est", [False, True])
@pytest.mark.parametrize("inv_s", ref.PARITY_INV_S)
@pytest.mark.parametrize("lds_row", [256, 512, 1024])
def test_parity_inputs_meet_the_preconditions(lds_row, inv_s, est):
    m = 9
    depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(lds_row, m))
    r64 = ref.stage(depth, sdf, pi, cref.shared_u(m), float(inv_s), est, torch.float64)
    ref.check_preconditions(r64, pi)
    print(f"L={lds_row} inv_s={inv_s} est={est}: min wsum (len >= 17) {r64['wsum'][pi[:, 1] >= 17].min().item():.6f}, "
          f"transmittance margin {r64['t_margin'].min().item():.3e}")
    exact = ref.exact_packs(r64, pi)
    assert exact[pi[:, 1] <= 2].all(), "packs of one and two elements carry no mass here"
    r32 = ref.stage(depth, sdf, pi, cref.shared_u(m), float(inv_s), est, torch.float32)
    assert torch.equal(r32['fine'][exact].double(), r64['fine'][exact])
