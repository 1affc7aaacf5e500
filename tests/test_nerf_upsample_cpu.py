"""The two packed stages of the NeRF march + up-sample ray query without a GPU: the restatement the GPU tests measure the HIP kernels
against (tests/nerf_upsample_ref.py) anchored to the CPU oracle's pack ops, the ABI entries, the driver's refusal of CPU tensors,
and the preconditions of the GPU parity cases asserted on their inputs.

Anchor.  Both sides get the same float32 opacities.  The oracle's chain is packed_cumsum (added in order in float32, as the
restatement's sum), a float32 division by max(last, 1e-5), packed_invert_cdf, try_merge_two_packs_sorted_aligned and packed_diff.
Sum, CDF and the bin found are the same float32 operations in the same order on both sides; the lerp is one fma on both, the
restatement's through a float64 product that is rounded twice, and the restatement raises a row to its running maximum, which moves
a value by the last rounding of that fma at the most: `fine` may differ by one ulp of the depth and nothing else may differ at all.

Preconditions.  The parity packs are uniform depths in [NEAR, FAR] through the soft shell of nerf_upsample_ref.shell_sigma on the rays
of fan_rays(4): every ray crosses the shell twice.  The shell is not the 60 exp(-((|x| - 0.62) / 0.08)^2) one would write first: with
that one the CDF rests on 1/2 between the two crossings and on small fractions in the short packs, which are CDF positions (18 of the
36 cases below broke a rule); the peak of 3 and the skew along z are what keeps every case inside the rules.  Packs of one and
two elements carry no mass (their samples lie outside the shell, the last element of a pack has no interval) and come out exactly;
the margins of the others are printed per case."""
import numpy as np
import pytest
import torch

import neus_coarse_ref as cref
import nerf_upsample_ref as ref
from nr3d_lib_amd import _abi

LENGTHS = [1, 2, 3, 5, 17, 33, 63, 64, 65, 128, 129, 200, 487, 488, 1031]


def _coarse_of(P, nc):
    return ref.coarse_rows(torch.full((P,), cref.NEAR), torch.full((P,), cref.FAR), nc)


@pytest.mark.parametrize("per_pack", [False, True])
@pytest.mark.parametrize("m", [9, 65])
def test_stage_restatement_matches_oracle_chain(oracle, m, per_pack):
    depth, sigma, delta, pi, _, _ = ref.soft_shell_packs(LENGTHS)
    P, nc = pi.shape[0], 16
    u = ref.per_pack_u(P, m) if per_pack else ref.shared_u(m)
    coarse = _coarse_of(P, nc)
    r = ref.stage(depth, sigma, delta, pi, u, coarse=coarse, dtype=torch.float32)
    alpha, pinfo = r['alpha'].numpy(), pi.numpy()
    assert alpha.dtype == np.float32
    c = oracle.packed_cumsum(alpha, pinfo)
    last = c[pinfo[:, 0] + pinfo[:, 1] - 1]
    cdf = (c / np.repeat(np.maximum(last, np.float32(1e-5)), pinfo[:, 1])).astype(np.float32)
    mask = ref.padded(pi, depth.shape[0])[1]
    np.testing.assert_array_equal(cdf, r['cdf'][mask].numpy())
    fine, bins = oracle.packed_invert_cdf(depth.numpy(), cdf, np.ascontiguousarray(np.broadcast_to(u.numpy(), (P, m))), pinfo)
    np.testing.assert_array_equal(bins, (pi[:, :1] + r['pos']).numpy())            # the same bin found
    ulp = np.spacing(np.abs(fine).astype(np.float32))
    assert (np.abs(fine.astype(np.float64) - r['fine'].double().numpy()) <= ulp).all()
    # the union of the coarse rows with the restatement's own new depths: positions, packs and differences exactly
    own = r['fine'].numpy()
    pinfo_c = np.stack([np.arange(P) * nc, np.full(P, nc)], 1).astype(np.int64)
    pinfo_f = np.stack([np.arange(P) * m, np.full(P, m)], 1).astype(np.int64)
    pa, pb, pim = oracle.try_merge_two_packs_sorted_aligned(coarse.numpy().ravel(), pinfo_c, own.ravel(), pinfo_f, b_sorted=True)
    begin = (torch.arange(P) * (nc + m))[:, None]
    np.testing.assert_array_equal(pa.reshape(P, nc), (begin + r['pos_coarse']).numpy())
    np.testing.assert_array_equal(pb.reshape(P, m), (begin + r['pos_fine']).numpy())
    np.testing.assert_array_equal(pim, np.stack([np.arange(P) * (nc + m), np.full(P, nc + m)], 1))
    merged = np.empty(P * (nc + m), np.float32)
    merged[pa], merged[pb] = coarse.numpy().ravel(), own.ravel()
    np.testing.assert_array_equal(merged.reshape(P, nc + m), r['merged'].numpy())
    np.testing.assert_array_equal(oracle.packed_diff(merged, pim).reshape(P, nc + m), r['deltas'].numpy())
    assert (np.diff(merged.reshape(P, nc + m), axis=-1) >= 0).all()
    # and without a coarse row: the interval ends
    r0 = ref.stage(depth, sigma, delta, pi, u, dtype=torch.float32)
    assert torch.equal(r0['fine'], r['fine']) and torch.equal(r0['deltas'], r['fine'].diff(dim=-1))
    assert torch.equal(r0['merged'], r['fine'][:, :-1] + r['fine'].diff(dim=-1))


def _merge_case(nc=16):
    """rays with and without a marched pack (the first and the last without), marched depths equal to coarse ones among them"""
    lens = torch.tensor([0, 1, 63, 0, 64, 65, 0, 0, 515, 5, 0], dtype=torch.int64)
    R = lens.numel()
    pi_all = torch.stack([torch.cumsum(lens, 0) - lens, lens], -1)
    rays = cref.fan_rays(4)
    coarse = ref.coarse_rows(rays['near'][:R], rays['far'][:R], nc)
    which = torch.repeat_interleave(torch.arange(R), lens)
    k = (torch.arange(int(lens.sum())) - pi_all[which, 0]).float()
    depth = (1.7 + 1.5 * k / (lens - 1).clamp_min(1).float()[which]).float()
    # ties: the first marched samples of ray 4 and the last of ray 8 sit on coarse depths, one of them twice
    b4, b8 = int(pi_all[4, 0]), int(pi_all[8, 0] + pi_all[8, 1])
    below = coarse[4][coarse[4] < depth[b4 + 3]]
    depth[b4:b4 + 3] = torch.stack([below[-2], below[-1], below[-1]])
    depth[b8 - 2:b8] = coarse[8][-1]
    return coarse, depth.contiguous(), pi_all, rays['rays_o'][:R].contiguous(), rays['rays_d'][:R].contiguous()


def test_merge_restatement_matches_oracle_merge(oracle):
    coarse, depth, pi_all, o, v = _merge_case()
    R, nc = coarse.shape
    for s in range(R):
        b, n = pi_all[s].tolist()
        assert (depth[b:b + n].diff() >= 0).all()
    r = ref.merge(coarse, depth, pi_all, o, v)
    pinfo_c = np.stack([np.arange(R) * nc, np.full(R, nc)], 1).astype(np.int64)
    pa, pb, pim = oracle.try_merge_two_packs_sorted_aligned(coarse.numpy().ravel(), pinfo_c, depth.numpy(), pi_all.numpy(), b_sorted=True)
    np.testing.assert_array_equal(pa.reshape(R, nc), r['pidx_coarse'].numpy())
    np.testing.assert_array_equal(pb, r['pidx_marched'].numpy())
    np.testing.assert_array_equal(pim, r['pack_infos_out'].numpy())
    np.testing.assert_array_equal(oracle.packed_diff(r['depths_all'].numpy(), pim), r['deltas_all'].numpy())
    t = r['depths_all']
    first, n = r['pack_infos_out'][4].tolist()
    assert (t[first:first + n].diff() == 0).sum() >= 3, "the ties are there"
    for s in range(R):
        first, n = r['pack_infos_out'][s].tolist()
        assert (t[first:first + n].diff() >= 0).all() and (r['ridx_all'][first:first + n] == s).all()
    x64 = o.double()[r['ridx_all']] + v.double()[r['ridx_all']] * t.double()[:, None]
    assert (r['samples_all'].double() - x64).abs().max().item() <= float(np.spacing(np.float32(4.0)))


def test_a_marched_depth_goes_before_an_equal_coarse_one(oracle):
    a = torch.tensor([[1, 2, 2, 3, 5, 5]], dtype=torch.float32)
    b = torch.tensor([[0.5, 2, 2, 5, 6, 6]], dtype=torch.float32)
    pa, pb, _ = oracle.try_merge_two_packs_sorted_aligned(a.numpy().ravel(), np.array([[0, 6]]), b.numpy().ravel(), np.array([[0, 6]]),
                                                          b_sorted=True)
    pos_a, pos_b = ref.union_positions(a, b)
    np.testing.assert_array_equal(pa, pos_a[0].numpy())
    np.testing.assert_array_equal(pb, pos_b[0].numpy())
    assert pos_b[0].tolist() == [0, 2, 3, 7, 10, 11] and pos_a[0].tolist() == [1, 4, 5, 6, 8, 9]


def test_abi_lists_the_nerf_stages():
    assert _abi.ABI_VERSION >= 24
    assert _abi.SIGNATURES['nr3d_nerf_upsample_lds_row'] == ('int', [])
    ret, args = _abi.SIGNATURES['nr3d_nerf_merge_rows_packs']
    assert ret == 'int' and args == ['uint32_t', 'uint32_t', 'uint64_t'] + ['ptr'] * 10 + ['ptr']
    ret, args = _abi.SIGNATURES['nr3d_nerf_upsample_stage_packed']
    assert ret == 'int' and args == ['uint32_t', 'uint64_t', 'uint32_t', 'uint32_t', 'uint64_t'] + ['ptr'] * 5 + ['int64_t'] + ['ptr'] * 6 \
        + ['ptr']


def test_driver_and_bindings_refuse_cpu_tensors():
    """the package's ops run on the GPU only, the op-chain route of the driver included: a CPU ray batch raises the usual error"""
    import nr3d_lib_amd.graphics.nerf as nerf
    from nr3d_lib_amd.bindings import _nerf_upsample as U
    from nr3d_lib_amd.graphics.nerf import nerf_ray_query as rq
    assert nerf.nerf_ray_query_march_occ_multi_upsample_compressed is rq.nerf_ray_query_march_occ_multi_upsample_compressed
    assert isinstance(rq.FUSED_UPSAMPLE_NERF, bool)
    depth, sigma, delta, pi, o, v = ref.soft_shell_packs([5, 7])
    with pytest.raises(RuntimeError, match="GPU only"):
        U.upsample_stage_packed(depth, sigma, delta, pi, ref.shared_u(9))
    with pytest.raises(RuntimeError, match="GPU only"):
        U.merge_rows_packs(_coarse_of(2, 4), depth, pi, o, v)

    class Marched:
        ridx_hit, ridx = torch.arange(2), torch.repeat_interleave(torch.arange(2), pi[:, 1])
        pack_infos, depth_samples, deltas = pi, depth, delta
        samples = o[ridx] + v[ridx] * depth[:, None]

    class Accel:
        def ray_march(self, *a, **kw):
            return Marched

    class Model:
        accel = Accel()

        def query_density(self, x, **kw):
            return ref.shell_sigma(x)

        def forward(self, x, **kw):
            return dict(sigma=ref.shell_sigma(x), rgb=torch.sigmoid(x))

    rays = dict(num_rays=2, rays_o=o, rays_d=v, near=torch.full((2,), cref.NEAR), far=torch.full((2,), cref.FAR),
                rays_inds=torch.arange(2))
    for fused in (True, False):
        rq_fused = rq.FUSED_UPSAMPLE_NERF
        rq.FUSED_UPSAMPLE_NERF = fused
        try:
            with pytest.raises(RuntimeError, match="GPU only"):
                rq.nerf_ray_query_march_occ_multi_upsample_compressed(Model(), rays, num_coarse=4, num_fine=8)
        finally:
            rq.FUSED_UPSAMPLE_NERF = rq_fused


@pytest.mark.parametrize("per_pack", [False, True])
@pytest.mark.parametrize("nc", ref.PARITY_NC)
@pytest.mark.parametrize("m", ref.PARITY_M)
@pytest.mark.parametrize("lds_row", [256, 512, 1024])
def test_parity_inputs_meet_the_preconditions(lds_row, m, nc, per_pack):
    depth, sigma, delta, pi, _, _ = ref.soft_shell_packs(ref.parity_lengths(lds_row, m, nc))
    P = pi.shape[0]
    u = ref.per_pack_u(P, m) if per_pack else ref.shared_u(m)
    coarse = _coarse_of(P, nc) if nc else None
    r64 = ref.stage(depth, sigma, delta, pi, u, coarse=coarse, dtype=torch.float64)
    margins = ref.check_preconditions(r64, pi)
    print(f"L={lds_row} m={m} nc={nc} per_pack={per_pack}: min c_(n-1) over len >= 17 {margins['min_mass']:.4f}, "
          f"nearest u to a CDF value {margins['min_u_gap']:.3e}, nearest pmf to 1e-5 a factor {np.exp(margins['pmf_nearest']):.3g}")
    r32 = ref.stage(depth, sigma, delta, pi, u, coarse=coarse, dtype=torch.float32)
    assert torch.equal(r32['pos'], r64['pos']), "both runs invert the same bins"
    short = pi[:, 1] <= 2
    assert torch.equal(r32['fine'][short].double(), r64['fine'][short]), "packs of one and two elements come out exactly"
    # sigma = 0: every opacity is exactly 0, the pack has no mass and every position returns depth_(n-2) (depth_0 for one element)
    z32 = ref.stage(depth, torch.zeros_like(sigma), delta, pi, u, coarse=coarse, dtype=torch.float32)
    z64 = ref.stage(depth, torch.zeros_like(sigma), delta, pi, u, coarse=coarse, dtype=torch.float64)
    expect = depth[pi[:, 0] + (pi[:, 1] - 2).clamp_min(0)]
    assert torch.equal(z32['fine'], expect[:, None].expand(P, m)) and torch.equal(z32['fine'].double(), z64['fine'])
