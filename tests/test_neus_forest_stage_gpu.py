"""The block-carrying packed up-sampling stage (csrc/neus_upsample.hip, k_stage_packed<.., LABELS = true>) through
bindings._neus_upsample.upsample_stage_packed_blocks.

Inputs: the parity packs of tests/test_neus_upsample_packed_gpu.py (1 ... 2 L + 7 elements, L = PACKED_LDS_ROW, shuffled, so LDS
and global packs share workgroups and the last workgroup is partial), labels that change every 3 samples inside a pack.

1. Everything the unlabelled stage returns must be the same bits from both entries.
2. Structure, exactly: blidx_merged[pidx_fine] == blidx_fine, the remaining places of every pack hold the old labels in order.
3. blidx_fine against the float64 restatement (tests/neus_forest_ref.py).  The label is decided by the bin the inversion finds:
   a case (p, j) whose u_j lies within tau of a float64 CDF knot of its pack is a proven tie and may carry the label of pos64 - 1,
   pos64 or pos64 + 1; every other case must match.  tau = 4 x the largest |cdf32 - cdf64| of the restatement on the call's own
   inputs; at most 0.5 % of the cases may be ties.
4. Packs whose CDF is exactly 0 up to k* and exactly 1 after it, a label change between k* and k* + 1: no rounding can move that."""
import pytest
import torch

import neus_coarse_ref as cref
import neus_forest_ref as fref
import neus_packed_ref as ref
from nr3d_lib_amd.bindings import _neus_upsample as U

pytestmark = pytest.mark.gpu


def run(dev, depth, sdf, bl, pi, u, inv_s, est, **kw):
    out = U.upsample_stage_packed_blocks(depth.to(dev), sdf.to(dev), bl.to(dev), pi.to(dev), u.to(dev), inv_s, est, **kw)
    plain = U.upsample_stage_packed(depth.to(dev), sdf.to(dev), pi.to(dev), u.to(dev), inv_s, est, **kw)
    torch.cuda.synchronize()
    cpu = lambda ts: tuple(None if t is None else t.cpu() for t in ts)
    return cpu(out), cpu(plain)


def check_same_bits(out, plain):
    fine, bl_fine, merged, sdf_m, bl_m, pidx, pi_out = out
    p_fine, p_merged, p_sdf_m, p_pidx, p_pi_out = plain
    assert torch.equal(fine, p_fine), "fine"
    for name, a, b in (("merged", merged, p_merged), ("pidx_fine", pidx, p_pidx), ("pack_infos_out", pi_out, p_pi_out)):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), name
    assert (sdf_m is None) == (p_sdf_m is None)
    if sdf_m is not None:
        old = torch.ones(sdf_m.shape[0], dtype=torch.bool)
        old[pidx.flatten()] = False
        assert torch.equal(sdf_m[old], p_sdf_m[old]), "sdf_merged at the old places"


def check_structure(bl, pi, out):
    fine, bl_fine, merged, sdf_m, bl_m, pidx, pi_out = out
    P, m = fine.shape
    assert bl_fine.shape == (P, m) and bl_fine.dtype == torch.int64
    if merged is None:
        assert bl_m is None
        return
    assert bl_m.shape == merged.shape and bl_m.dtype == torch.int64
    assert torch.equal(bl_m[pidx], bl_fine), "blidx_merged[pidx_fine] != blidx_fine"
    old = torch.ones(bl_m.shape[0], dtype=torch.bool)
    old[pidx.flatten()] = False
    for p, (b, n) in enumerate(pi.tolist()):
        ob = b + p * m
        assert torch.equal(bl_m[ob:ob + n + m][old[ob:ob + n + m]], bl[b:b + n]), f"pack {p}: old labels moved"


def check_labels(depth, sdf, bl, pi, u, inv_s, est, bl_fine):
    """-> (cases, proven ties)"""
    r32 = fref.stage(depth, sdf, bl, pi, u, inv_s, est, torch.float32)
    r64 = fref.stage(depth, sdf, bl, pi, u, inv_s, est, torch.float64)
    tau = fref.cdf_tau(r32, r64)
    ties = fref.proven_ties(r64['cdf'], pi, u, tau)
    first, last = pi[:, :1], pi[:, :1] + pi[:, 1:] - 1
    near = [bl[torch.minimum(torch.maximum(first + r64['pos'] + k, first), last)] for k in (-1, 0, 1)]
    wrong = (bl_fine != near[1]) & ~ties
    print(f"P={pi.shape[0]} m={bl_fine.shape[1]} inv_s={inv_s} est={est}: {int(ties.sum())} proven ties of {ties.numel()}, tau {tau:.2e}, "
          f"{int((bl_fine != near[1]).sum())} labels differ from the float64 run's")
    assert not wrong.any(), f"{int(wrong.sum())} labels differ from the float64 restatement away from every CDF knot"
    assert ((bl_fine == near[0]) | (bl_fine == near[1]) | (bl_fine == near[2]))[ties].all(), "a tie carries a label two bins away"
    assert ties.sum().item() <= 0.005 * ties.numel(), "too many ties for the comparison to mean anything"
    return ties.numel(), int(ties.sum())


@pytest.mark.parametrize("inv_s", ref.PARITY_INV_S)
@pytest.mark.parametrize("est", [False, True])
@pytest.mark.parametrize("m", ref.PARITY_M)
def test_parity(dev, m, est, inv_s):
    depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(U.PACKED_LDS_ROW, m))
    bl = fref.labels_every(pi)
    u = cref.shared_u(m)
    out, plain = run(dev, depth, sdf, bl, pi, u, float(inv_s), est)
    check_same_bits(out, plain)
    check_structure(bl, pi, out)
    check_labels(depth, sdf, bl, pi, u, float(inv_s), est, out[1])


@pytest.mark.parametrize("est", [False, True])
def test_per_pack_u_and_labels_above_2_40(dev, est):
    m = 33
    depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(U.PACKED_LDS_ROW, m))
    bl = fref.labels_every(pi, base=2 ** 40 + 3)                 # a 32-bit path would cut these
    P = pi.shape[0]
    g = torch.Generator().manual_seed(7)
    u = ((torch.arange(m) + torch.rand(P, m, generator=g)) / m).contiguous()          # stratified, hence sorted
    out, plain = run(dev, depth, sdf, bl, pi, u, 256.0, est)
    check_same_bits(out, plain)
    check_structure(bl, pi, out)
    check_labels(depth, sdf, bl, pi, u, 256.0, est, out[1])
    assert (out[1] >= 2 ** 40).all() and (out[4] >= 2 ** 40).all()


def test_merge_and_sdf_flags(dev):
    m = 9
    depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(U.PACKED_LDS_ROW, m))
    bl = fref.labels_every(pi)
    u = cref.shared_u(m)
    full, _ = run(dev, depth, sdf, bl, pi, u, 256.0, True)
    for kw in (dict(merge=False, need_sdf=False), dict(merge=False)):
        bare, plain = run(dev, depth, sdf, bl, pi, u, 256.0, True, **kw)
        check_same_bits(bare, plain)
        assert torch.equal(bare[0], full[0]) and torch.equal(bare[1], full[1]) and all(t is None for t in bare[2:])
    no_sdf, plain = run(dev, depth, sdf, bl, pi, u, 256.0, True, need_sdf=False)
    check_same_bits(no_sdf, plain)
    check_structure(bl, pi, no_sdf)
    assert no_sdf[3] is None and all(torch.equal(a, b) for a, b in zip(no_sdf, full) if a is not None)


def test_no_packs(dev):
    e = torch.empty(0)
    out, _ = run(dev, e, e, torch.empty(0, dtype=torch.int64), torch.empty(0, 2, dtype=torch.int64), cref.shared_u(9), 64.0, False)
    fine, bl_fine, merged, sdf_m, bl_m, pidx, pi_out = out
    assert fine.shape == bl_fine.shape == (0, 9) and merged.shape == sdf_m.shape == bl_m.shape == (0,)
    assert pidx.shape == (0, 9) and pi_out.shape == (0, 2) and bl_fine.dtype == bl_m.dtype == torch.int64


@pytest.mark.parametrize("est", [False, True])
def test_label_change_at_an_exact_cdf_step(dev, est):
    """SDF +100 up to k*, -100 after: the CDF is exactly 0 up to k* and exactly 1 after it in float32 as in float64 (one weight, divided
    by itself), so every u in (0, 1) finds pos = k* + 1.  The label changes between k* and k* + 1."""
    L, m = U.PACKED_LDS_ROW, 9
    cases = [(2, 0), (40, 0), (40, 19), (40, 38), (130, 63), (130, 64), (130, 128), (L + 30, 63), (L + 30, 64), (L + 30, L + 28)]
    depth, sdf, bl, first = [], [], [], 0
    pi = torch.empty(len(cases), 2, dtype=torch.int64)
    for p, (n, k) in enumerate(cases):
        depth.append(torch.arange(n, dtype=torch.float32) * 0.05 + 1.0)
        sdf.append(torch.where(torch.arange(n) <= k, torch.tensor(100.0), torch.tensor(-100.0)))
        bl.append(torch.where(torch.arange(n) <= k, 10 * p + 1, 10 * p + 2))
        pi[p, 0], pi[p, 1] = first, n
        first += n
    depth, sdf, bl = torch.cat(depth), torch.cat(sdf), torch.cat(bl)
    u = cref.shared_u(m)
    r64 = fref.stage(depth, sdf, bl, pi, u, 64.0, est, torch.float64)
    for p, (n, k) in enumerate(cases):
        b = int(pi[p, 0])
        assert torch.equal(r64['cdf'][b:b + n], (torch.arange(n) > k).double()), "the case is not what it claims to be"
    out, plain = run(dev, depth, sdf, bl, pi, u, 64.0, est)
    check_same_bits(out, plain)
    check_structure(bl, pi, out)
    want = torch.tensor([[10 * p + 2] * m for p in range(len(cases))])
    assert torch.equal(out[1], want), "a new depth did not take the label of the upper end of its bin"


def test_argument_checks(dev):
    depth, sdf, pi = ref.sphere_packs([17, 5, 33])
    bl = fref.labels_every(pi)
    d, s, b, p, u = depth.to(dev), sdf.to(dev), bl.to(dev), pi.to(dev), cref.shared_u(9).to(dev)
    f = U.upsample_stage_packed_blocks
    with pytest.raises(RuntimeError, match="GPU only"):
        f(d, s, bl, p, u, 64.0, False)
    with pytest.raises(RuntimeError, match="`blidx` must be a tensor"):
        f(d, s, None, p, u, 64.0, False)
    with pytest.raises(RuntimeError, match="`blidx` must be int64"):
        f(d, s, b.int(), p, u, 64.0, False)
    with pytest.raises(RuntimeError, match="`blidx` must be"):
        f(d, s, b[:-1].contiguous(), p, u, 64.0, False)
    with pytest.raises(RuntimeError, match="contiguous"):
        f(d, s, b.repeat_interleave(2)[::2], p, u, 64.0, False)
    with pytest.raises(RuntimeError, match="float32"):
        f(d.double(), s, b, p, u, 64.0, False)
    with pytest.raises(RuntimeError, match="`pack_infos` must be int64"):
        f(d, s, b, p.int(), u, 64.0, False)
    with pytest.raises(RuntimeError, match=r"`pack_infos` must be \[P, 2\]"):
        f(d, s, b, p.flatten(), u, 64.0, False)
    with pytest.raises(RuntimeError, match="`u` must be"):
        f(d, s, b, p, u.expand(2, 9).contiguous(), 64.0, False)
