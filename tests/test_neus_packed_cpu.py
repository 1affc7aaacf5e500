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
    # one entry for packs with and without labels (ABI 28): blidx after sdf, blidx_fine after fine, blidx_merged after sdf_merged
    assert ret == 'int' and args == ['uint32_t', 'uint64_t', 'uint32_t'] + ['ptr'] * 5 + ['int64_t', 'float', 'int', 'int', 'int'] \
        + ['ptr'] * 8 + ['ptr']
    assert 'nr3d_neus_upsample_stage_packed_blocks' not in _abi.SIGNATURES
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


def test_entry_refuses_before_any_launch(hiplib):
    """every rule of nr3d_neus_upsample_stage_packed that is checked before a launch, by its nr3d_last_error text.  Pointers that have
    to be non-NULL point at host scratch: a refused call touches none of them."""
    import ctypes
    scratch = (ctypes.c_char * 64)()
    X = ctypes.addressof(scratch)

    def call(P=1, N=8, m=9, blidx=None, u_stride=0, merge=0, need_sdf=0, blidx_fine=None, blidx_merged=None):
        # P, N, m, depth, sdf, blidx, pack_infos, u, u_stride, inv_s, use_estimate, merge, need_sdf, cdf_workspace, fine, blidx_fine,
        # merged, sdf_merged, blidx_merged, pidx_fine, pack_infos_out, stream: every tensor but the labels NULL
        return hiplib.nr3d_neus_upsample_stage_packed(P, N, m, None, None, blidx, None, None, u_stride, 64.0, 0, merge, need_sdf, None, None,
                                                      blidx_fine, None, None, blidx_merged, None, None, None)

    def refused(text, **kw):
        assert call(**kw) != 0
        assert text in hiplib.nr3d_last_error(), hiplib.nr3d_last_error()

    refused(b"m = 0, at least 1 new depth per pack", m=0)
    refused(b"u_stride = 3, must be 0 (one shared row) or m = 9", u_stride=3)
    assert call(u_stride=9) != 0 and b"NULL tensor pointer" in hiplib.nr3d_last_error()          # m itself passes that rule
    refused(b"need_sdf without merge", need_sdf=1)
    refused(b"the merged buffer holds at most 2^31 - 1 elements", P=2 ** 20, N=0, m=2 ** 11)
    refused(b"the merged buffer holds at most 2^31 - 1 elements", P=1, N=2 ** 31 - 9, m=9)
    refused(b"the merged buffer holds at most 2^31 - 1 elements", P=0, N=2 ** 31, m=9)
    refused(b"blidx without blidx_fine", blidx=X)
    refused(b"blidx without blidx_fine", blidx=X, blidx_merged=X, merge=1)
    refused(b"blidx_fine or blidx_merged without blidx", blidx_fine=X)
    refused(b"blidx_fine or blidx_merged without blidx", blidx_merged=X, merge=1)
    refused(b"merge with blidx but without blidx_merged", blidx=X, blidx_fine=X, merge=1)
    # the label rules come before the pointers are looked at, and P == 0 before that: a no-op with everything NULL
    assert call(P=0, N=0) == 0 and call(P=0, N=0, merge=1, need_sdf=1) == 0
    assert call(blidx=X, blidx_fine=X) != 0 and b"NULL tensor pointer" in hiplib.nr3d_last_error()
    assert all(b == b"\x00" for b in scratch), "a refused call wrote nothing"
