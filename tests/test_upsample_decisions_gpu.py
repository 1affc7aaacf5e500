"""GPU: the up-sampling stages on inputs that reach every clamp, floor and stop (tests/upsample_decision_inputs.py): k_stage and
k_stage_packed of csrc/neus_upsample.hip, the packed stage of csrc/nerf_upsample.hip with and without coarse rows, and k_invert_cdf of
csrc/pack_ops.hip, which carries the same inversion rule.

Values: `fine` against the float64 run of the restatement on the same float32 inputs, pack by pack: with e_ref_p = max |float32
restatement - float64 restatement| over pack p the kernel may be 4 e_ref_p + one ulp of the largest depth away, no element left out;
packs of one element and packs whose float64 mass is below 1e-7 exactly.  Each check prints a YARDSTICK line (the worst pack's
error / allowed).  tests/test_upsample_decisions_cpu.py shows that a kernel with one constant moved by a factor 10, or one rule
replaced, is 10 x allowed and more away on at least one of these packs.
Structure: the checks of the parity files on the kernel's own `fine` -- permutation, tie order, old depths unmoved, sdf_merged,
pack_infos_out; the union with the coarse rows and its differences.
Fused against composed: the packed NeuS and NeRF stages against the same stage composed from the library's own HIP pack ops (the
route the drivers take with the fused switch off) -- the one place where the three hand-written copies of the inversion rule meet.
The composed result is held to the same yardstick, and where a pack is exact both must agree bit for bit.
Every case runs twice and the bytes are compared."""
import json

import pytest
import torch

import nerf_upsample_ref as nref
import upsample_decision_inputs as D
from test_nerf_upsample_gpu import _check_outputs as nerf_structure
from test_neus_upsample_gpu import check_structure as rows_structure
from test_neus_upsample_packed_gpu import check_structure as packed_structure

pytestmark = pytest.mark.gpu

ROW_CASES = [(f, est, R, n) for f in D.PACKED_FAMILIES for est in D.estimates_of(f) for R, n in D.ROW_SHAPES]
PACKED_CASES = [(f, est) for f in D.PACKED_FAMILIES for est in D.estimates_of(f)]
NERF_CASES = [(f, nc) for f in D.NERF_FAMILIES for nc in nref.PARITY_NC]


def yardstick(check, case, c, fine):
    """per pack: |fine - float64 run| <= 4 e_ref_p + ulp, exact packs bit for bit; prints the worst pack"""
    fine = fine.cpu()
    err = D.per_pack_error(fine, c['r64']['fine'])
    ratio = err / c['allowed']
    p = int(ratio.argmax())
    print("YARDSTICK " + json.dumps(dict(check=check, case=[str(k) for k in case], packs=int(err.shape[0]), worst_pack=p,
                                         error=err[p].item(), allowed=c['allowed'][p].item(), ratio=ratio[p].item(),
                                         exact_packs=int(c['exact'].sum()))))
    assert torch.isfinite(fine).all(), f"{check} {case}: a new depth is not finite"
    assert (err <= c['allowed']).all(), f"{check} {case}: pack {p} is {ratio[p].item():.3g} x its allowed error away"
    assert torch.equal(fine[c['exact']].double(), c['r64']['fine'][c['exact']]), f"{check} {case}: a pack of one element or without mass"


def same_bytes(a, b, skip=()):
    for i, (x, y) in enumerate(zip(a, b)):
        if i not in skip and x is not None:
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


# ---- NeuS rows ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,est,R,n", ROW_CASES)
def test_rows_stage(dev, family, est, R, n):
    from nr3d_lib_amd.bindings import _neus_upsample as U
    c = D.rows_case(family, R, n, est)
    args = (c['depth'].to(dev), c['sdf'].to(dev), c['u'].to(dev), c['inv_s'], est)
    out = U.upsample_stage(*args)
    again = U.upsample_stage(*args)
    torch.cuda.synchronize()
    fine, merged, order = (t.cpu() for t in out)
    yardstick("rows", (family, est, R, n), c, fine)
    rows_structure(c['depth'], fine, merged, order)
    same_bytes(out, again)


# ---- NeuS packs --------------------------------------------------------------------------------------------------------------------

def _packed_case(family, est):
    from nr3d_lib_amd.bindings import _neus_upsample as U
    return D.packed_case(family, U.PACKED_LDS_ROW, est)


@pytest.mark.parametrize("family,est", PACKED_CASES)
def test_packed_stage(dev, family, est):
    from nr3d_lib_amd.bindings import _neus_upsample as U
    c = _packed_case(family, est)
    assert (c['pi'][:, 1] + D.M > U.PACKED_LDS_ROW).any() and (c['pi'][:, 1] + D.M <= U.PACKED_LDS_ROW).any(), "both address spaces"
    args = (c['depth'].to(dev), c['sdf'].to(dev), c['pi'].to(dev), c['u'].to(dev), c['inv_s'], est)
    out = U.upsample_stage_packed(*args)
    again = U.upsample_stage_packed(*args)
    torch.cuda.synchronize()
    yardstick("packed", (family, est), c, out[0])
    packed_structure(c['depth'], c['sdf'], c['pi'], *(t.cpu() for t in out))
    new = torch.zeros(out[1].shape[0], dtype=torch.bool, device=dev)
    new[out[3].flatten()] = True
    same_bytes(out, again, skip=(2,))
    assert torch.equal(out[2][~new], again[2][~new])            # the places of the new depths in sdf_merged are the caller's


def _composed_neus(depth, sdf, pi, u, inv_s, est):
    """the stage as the march-occ drivers run it with FUSED_UPSAMPLE_PACKED off, on the library's HIP pack ops"""
    from nr3d_lib_amd.graphics.neus.neus_utils import neus_packed_sdf_to_alpha, neus_packed_sdf_to_upsample_alpha
    from nr3d_lib_amd.graphics.pack_ops import packed_alpha_to_vw, packed_cumsum, packed_div, packed_invert_cdf
    alpha = neus_packed_sdf_to_upsample_alpha(sdf, depth, inv_s, pi) if est else neus_packed_sdf_to_alpha(sdf, inv_s, pi, fused=False)
    cdf = packed_cumsum(packed_alpha_to_vw(alpha, pi), pi, exclusive=True)
    last = cdf[pi[..., 0] + pi[..., 1] - 1]
    cdf = packed_div(cdf, last.clamp_min(1e-5), pi)
    return packed_invert_cdf(depth, cdf.to(depth.dtype), u.contiguous(), pi)[0]


@pytest.mark.parametrize("family,est", PACKED_CASES)
def test_packed_stage_fused_against_composed(dev, family, est):
    from nr3d_lib_amd.bindings import _neus_upsample as U
    c = _packed_case(family, est)
    depth, sdf, pi, u = c['depth'].to(dev), c['sdf'].to(dev), c['pi'].to(dev), c['u'].to(dev)
    fused = U.upsample_stage_packed(depth, sdf, pi, u, c['inv_s'], est, merge=False)[0]
    composed = _composed_neus(depth, sdf, pi, u, c['inv_s'], est)
    again = _composed_neus(depth, sdf, pi, u, c['inv_s'], est)
    torch.cuda.synchronize()
    assert torch.equal(composed.view(torch.int32), again.view(torch.int32))
    composed = torch.cummax(composed, -1).values                # the fused stage raises a row to its running maximum
    yardstick("packed composed", (family, est), c, composed)
    yardstick("packed fused", (family, est), c, fused)
    exact = c['exact'].to(dev)
    assert torch.equal(fused[exact], composed[exact]), "exact packs: fused and composed differ"
    apart = (fused.double() - composed.double()).abs().amax(-1).cpu()
    print(f"packed {family} est={est}: fused and composed {(apart / c['allowed']).max().item():.3g} x allowed apart at the most")


# ---- NeRF --------------------------------------------------------------------------------------------------------------------------

def _nerf_case(family, nc):
    from nr3d_lib_amd.bindings import _nerf_upsample as U
    return D.nerf_case(family, U.LDS_ROW, nc)


def _to(dev, c, *names):
    return [None if c.get(k) is None else c[k].to(dev) for k in names]


@pytest.mark.parametrize("family,nc", NERF_CASES)
def test_nerf_stage(dev, family, nc):
    from nr3d_lib_amd.bindings import _nerf_upsample as U
    c = _nerf_case(family, nc)
    lens = c['pi'][:, 1] + D.M + nc
    assert (lens > U.LDS_ROW).any() and (lens <= U.LDS_ROW).any(), "both address spaces"
    depth, sigma, delta, pi, u, coarse, row = _to(dev, c, 'depth', 'sigma', 'delta', 'pi', 'u', 'coarse', 'row')
    out = U.upsample_stage_packed(depth, sigma, delta, pi, u, coarse=coarse, coarse_row=row)
    again = U.upsample_stage_packed(depth, sigma, delta, pi, u, coarse=coarse, coarse_row=row)
    torch.cuda.synchronize()
    yardstick("nerf", (family, nc), c, out[0])
    nerf_structure(*out, coarse, row, nc, D.M)
    same_bytes(out, again)


def _composed_nerf(depth, sigma, delta, pi, u):
    """the stage as the NeRF driver runs it with FUSED_UPSAMPLE_NERF off, on the library's HIP pack ops"""
    from nr3d_lib_amd.graphics.nerf.nerf_utils import tau_to_alpha
    from nr3d_lib_amd.graphics.pack_ops import packed_cumsum, packed_div, packed_invert_cdf
    cdf = packed_cumsum(tau_to_alpha(sigma * delta), pi)
    last = cdf[pi[..., 0] + pi[..., 1] - 1]
    cdf = packed_div(cdf, last.clamp_min(1e-5), pi)
    return packed_invert_cdf(depth, cdf.to(depth.dtype), u.contiguous(), pi)[0]


@pytest.mark.parametrize("family", D.NERF_FAMILIES)
def test_nerf_stage_fused_against_composed(dev, family):
    from nr3d_lib_amd.bindings import _nerf_upsample as U
    c = _nerf_case(family, 0)
    depth, sigma, delta, pi, u = _to(dev, c, 'depth', 'sigma', 'delta', 'pi', 'u')
    fused = U.upsample_stage_packed(depth, sigma, delta, pi, u)[0]
    composed = _composed_nerf(depth, sigma, delta, pi, u)
    again = _composed_nerf(depth, sigma, delta, pi, u)
    torch.cuda.synchronize()
    assert torch.equal(composed.view(torch.int32), again.view(torch.int32))
    composed = torch.cummax(composed, -1).values
    yardstick("nerf composed", (family,), c, composed)
    yardstick("nerf fused", (family,), c, fused)
    exact = c['exact'].to(dev)
    assert torch.equal(fused[exact], composed[exact]), "exact packs: fused and composed differ"
    apart = (fused.double() - composed.double()).abs().amax(-1).cpu()
    print(f"nerf {family}: fused and composed {(apart / c['allowed']).max().item():.3g} x allowed apart at the most")


# ---- packed_invert_cdf -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", D.INVERT_FAMILIES)
def test_packed_invert_cdf(dev, family):
    from nr3d_lib_amd.bindings import _nerf_upsample as U
    from nr3d_lib_amd.graphics.pack_ops import packed_invert_cdf
    c = D.invert_case(family, U.LDS_ROW)
    bins, cdf, u, pi = _to(dev, c, 'depth', 'cdf', 'u', 'pi')
    out = packed_invert_cdf(bins, cdf, u, pi)
    again = packed_invert_cdf(bins, cdf, u, pi)
    torch.cuda.synchronize()
    yardstick("invert", (family,), c, out[0])
    # the bin of every sample: the first CDF value at or above u, the pack's last element when there is none
    samples, bin_idx = out[0].cpu(), out[1].cpu()
    for p, (b, n) in enumerate(c['pi'].tolist()):
        want = b + torch.searchsorted(c['cdf'][b:b + n].contiguous(), c['u'][p].contiguous(), right=False).clamp_max(n - 1)
        assert torch.equal(bin_idx[p], want), f"pack {p}: bins"
        lo, hi = c['depth'][(bin_idx[p] - 1).clamp_min(b)], c['depth'][bin_idx[p]]
        assert ((samples[p] >= lo) & (samples[p] <= hi + D.ulp_of(c['depth']))).all(), f"pack {p}: a sample outside its bin"
    same_bytes(out, again)
