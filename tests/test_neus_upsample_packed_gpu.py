"""The packed up-sampling stage (csrc/neus_upsample.hip, k_stage_packed) through bindings._neus_upsample.upsample_stage_packed.

One call holds packs of 1, 2, 3, 5, 17, 33, 63, 64, 65, 128, 129, 200, L - m, L - m + 1 and 2 L + 7 elements (L = PACKED_LDS_ROW) in a
shuffled order: the chunk boundaries of the wave scans, the last pack that is staged in LDS, the first that is not, and a long one on
global memory, LDS and global packs side by side in the same workgroups.

Values: `fine` against the float64 run of the restatement (tests/neus_packed_ref.py) on the same float32 inputs, under the rule of
tests/test_neus_upsample_gpu.py: e_ref = max |float32 restatement - float64 restatement| over the call, and the kernel may be
4 e_ref plus one ulp of the largest depth away (it associates its products and sums as a tree where the restatement goes left to
right).  The comparison needs decisions that rounding cannot flip, which the parity cases assert on the float64 run
(neus_packed_ref.check_preconditions): weight sum >= 0.99 for packs of 17 elements and more, no transmittance within 0.1 % of the
early stop, no inverted bin with a pmf in [0.5e-5, 2e-5].  Packs of one element and packs without mass are compared exactly.
Structure: the union, its positions and the SDF are checked exactly on the kernel's own `fine`."""
import numpy as np
import pytest
import torch

import neus_coarse_ref as cref
import neus_packed_ref as ref
from nr3d_lib_amd.bindings import _neus_upsample as U

pytestmark = pytest.mark.gpu


def run(dev, depth, sdf, pi, u, inv_s, est, **kw):
    out = U.upsample_stage_packed(depth.to(dev), sdf.to(dev), pi.to(dev), u.to(dev), inv_s, est, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in out)


def check_structure(depth, sdf, pi, fine, merged, sdf_merged, pidx_fine, pi_out):
    P, m = fine.shape
    N = depth.shape[0]
    assert merged.shape == (N + P * m,) and pidx_fine.shape == (P, m) and pidx_fine.dtype == torch.int64
    assert torch.equal(pi_out, torch.stack([pi[:, 0] + torch.arange(P) * m, pi[:, 1] + m], 1)), "pack_infos_out"
    assert torch.equal(merged[pidx_fine], fine), "merged[pidx_fine] != fine"
    is_new = torch.zeros(N + P * m, dtype=torch.bool)
    is_new[pidx_fine.flatten()] = True
    for p, (b, n) in enumerate(pi.tolist()):
        ob = b + p * m
        row, new = merged[ob:ob + n + m], is_new[ob:ob + n + m]
        assert torch.equal(row, torch.cat([depth[b:b + n], fine[p]]).sort().values), f"pack {p}: merged is not sort(cat(depth, fine))"
        assert int(new.sum()) == m and (pidx_fine[p] >= ob).all() and (pidx_fine[p] < ob + n + m).all(), f"pack {p}: no permutation"
        assert (pidx_fine[p].diff() > 0).all(), f"pack {p}: equal new depths out of order"
        assert torch.equal(row[~new], depth[b:b + n]), f"pack {p}: old depths moved"
        tie = row[1:] == row[:-1]
        assert not (tie & ~new[:-1] & new[1:]).any(), f"pack {p}: an old depth precedes an equal new one"
        if sdf_merged is not None:
            assert torch.equal(sdf_merged[ob:ob + n + m][~new], sdf[b:b + n]), f"pack {p}: sdf_merged"


def check_values(depth, sdf, pi, u, inv_s, est, fine, preconditions=False):
    r32 = ref.stage(depth, sdf, pi, u, inv_s, est, torch.float32)
    r64 = ref.stage(depth, sdf, pi, u, inv_s, est, torch.float64)
    if preconditions:
        ref.check_preconditions(r64, pi)
    e_ref = (r32['fine'].double() - r64['fine']).abs().max().item()
    err = (fine.double() - r64['fine']).abs().max().item()
    ulp = float(np.spacing(np.float32(depth.abs().max().item())))
    print(f"P={pi.shape[0]} m={fine.shape[1]} inv_s={inv_s} est={est}: kernel {err:.3e}  e_ref {e_ref:.3e}  allowed {4 * e_ref + ulp:.3e}")
    assert torch.isfinite(fine).all()
    assert err <= 4 * e_ref + ulp
    exact = ref.exact_packs(r64, pi)
    assert torch.equal(fine[exact].double(), r64['fine'][exact]), "a pack of one element or without mass"
    return r32


@pytest.mark.parametrize("inv_s", ref.PARITY_INV_S)
@pytest.mark.parametrize("est", [False, True])
@pytest.mark.parametrize("m", ref.PARITY_M)
def test_parity(dev, m, est, inv_s):
    L = U.PACKED_LDS_ROW
    assert L in (256, 512, 1024)
    depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(L, m))
    u = cref.shared_u(m)
    out = run(dev, depth, sdf, pi, u, float(inv_s), est)
    check_values(depth, sdf, pi, u, float(inv_s), est, out[0], preconditions=True)
    check_structure(depth, sdf, pi, *out)


@pytest.mark.parametrize("est", [False, True])
def test_one_element_and_massless_packs(dev, est):
    m = 9
    lengths = [1, 2, 1, 40, 1, U.PACKED_LDS_ROW + 3]
    depth, _, pi = ref.sphere_packs(lengths)
    sdf = (1.0 + 0.25 * (depth - 2.5).abs()).contiguous()                             # never below 1: every alpha is exactly 0
    out = run(dev, depth, sdf, pi, cref.shared_u(m), 64.0, est)
    for p, (b, n) in enumerate(pi.tolist()):
        assert torch.equal(out[0][p], depth[b + max(n - 2, 0)].expand(m)), f"pack {p} of {n}"
    check_structure(depth, sdf, pi, *out)


@pytest.mark.parametrize("est", [False, True])
def test_zero_length_span(dev, est):
    m = 9
    lengths = [17, 1, 65, U.PACKED_LDS_ROW + 3]
    depth, sdf, pi = ref.sphere_packs(lengths, near=2.0, far=2.0)
    u = cref.shared_u(m)
    out = run(dev, depth, sdf, pi, u, 64.0, est)
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()
    assert torch.equal(out[0], ref.stage(depth, sdf, pi, u, 64.0, est, torch.float32)['fine'])
    check_structure(depth, sdf, pi, *out)


@pytest.mark.parametrize("est", [False, True])
def test_per_pack_u(dev, est):
    m = 33
    depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(U.PACKED_LDS_ROW, m))
    P = pi.shape[0]
    g = torch.Generator().manual_seed(7)
    u = ((torch.arange(m) + torch.rand(P, m, generator=g)) / m).contiguous()          # stratified, hence sorted
    out = run(dev, depth, sdf, pi, u, 256.0, est)
    check_values(depth, sdf, pi, u, 256.0, est, out[0])
    check_structure(depth, sdf, pi, *out)
    shared = run(dev, depth, sdf, pi, u[0].contiguous(), 256.0, est)[0]
    assert torch.equal(shared[0], out[0][0]) and not torch.equal(shared, out[0])


def test_merge_and_sdf_flags(dev):
    m = 9
    depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(U.PACKED_LDS_ROW, m))
    u = cref.shared_u(m)
    full = run(dev, depth, sdf, pi, u, 256.0, True)
    bare = run(dev, depth, sdf, pi, u, 256.0, True, merge=False, need_sdf=False)
    assert torch.equal(bare[0], full[0]) and all(t is None for t in bare[1:])
    bare = run(dev, depth, sdf, pi, u, 256.0, True, merge=False)
    assert torch.equal(bare[0], full[0]) and all(t is None for t in bare[1:])
    no_sdf = run(dev, depth, sdf, pi, u, 256.0, True, need_sdf=False)
    assert no_sdf[2] is None and all(torch.equal(a, b) for a, b in zip(no_sdf, full) if a is not None)
    check_structure(depth, sdf, pi, *no_sdf)


def test_same_bytes_run_after_run(dev):
    m = 65
    depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(U.PACKED_LDS_ROW, m) * 3)
    u = cref.shared_u(m)
    a, b = run(dev, depth, sdf, pi, u, 256.0, True), run(dev, depth, sdf, pi, u, 256.0, True)
    new = torch.zeros(a[1].shape[0], dtype=torch.bool)
    new[a[3].flatten()] = True
    assert all(torch.equal(x, y) for x, y in zip(a[:2] + a[3:], b[:2] + b[3:]))
    assert torch.equal(a[2][~new], b[2][~new])                 # the places of the new depths in sdf_merged are the caller's


def test_no_packs(dev):
    e = torch.empty(0)
    fine, merged, sdf_m, pidx, pi_out = run(dev, e, e, torch.empty(0, 2, dtype=torch.int64), cref.shared_u(9), 64.0, False)
    assert fine.shape == (0, 9) and merged.shape == sdf_m.shape == (0,) and pidx.shape == (0, 9) and pi_out.shape == (0, 2)


def test_argument_checks(dev):
    depth, sdf, pi = ref.sphere_packs([17, 5, 33])
    d, s, p, u = depth.to(dev), sdf.to(dev), pi.to(dev), cref.shared_u(9).to(dev)
    with pytest.raises(RuntimeError, match="GPU only"):
        U.upsample_stage_packed(depth, s, p, u, 64.0, False)
    with pytest.raises(RuntimeError, match="GPU only"):
        U.upsample_stage_packed(d, s, pi, u, 64.0, False)
    with pytest.raises(RuntimeError, match="float32"):
        U.upsample_stage_packed(d.double(), s, p, u, 64.0, False)
    with pytest.raises(RuntimeError, match="`pack_infos` must be int64"):
        U.upsample_stage_packed(d, s, p.int(), u, 64.0, False)
    with pytest.raises(RuntimeError, match="contiguous"):
        U.upsample_stage_packed(d, s.repeat_interleave(2)[::2], p, u, 64.0, False)
    with pytest.raises(RuntimeError, match="contiguous"):
        U.upsample_stage_packed(d, s, p.t().contiguous().t(), u, 64.0, False)
    with pytest.raises(RuntimeError, match="`sdf` must be"):
        U.upsample_stage_packed(d, s[:-1].contiguous(), p, u, 64.0, False)
    with pytest.raises(RuntimeError, match=r"`depth` must be \[N\]"):
        U.upsample_stage_packed(d[:, None].contiguous(), s, p, u, 64.0, False)
    with pytest.raises(RuntimeError, match=r"`pack_infos` must be \[P, 2\]"):
        U.upsample_stage_packed(d, s, p.flatten(), u, 64.0, False)
    with pytest.raises(RuntimeError, match="`u` must be"):
        U.upsample_stage_packed(d, s, p, u.expand(2, 9).contiguous(), 64.0, False)
    with pytest.raises(RuntimeError, match="`u` must be"):
        U.upsample_stage_packed(d, s, p, u[:0], 64.0, False)
