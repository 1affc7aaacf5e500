"""GPU: the two packed stages of the NeRF march + up-sample ray query (bindings._nerf_upsample over csrc/nerf_upsample.hip).

(b) ``upsample_stage_packed`` against the restatement of tests/nerf_upsample_ref.py, which tests/test_nerf_upsample_cpu.py pins to
the CPU oracle: the new depths against its float64 run under the project's rule -- e_ref = max |float32 run - float64 run|, allowed
4 e_ref + one ulp of the largest depth, all three printed -- and everything that involves no rounding exactly: packs of one element
and packs without density against the float32 run, the union, its differences and the interval ends against the kernel's own new
depths.  One call holds packs of 1 ... 2 L + 7 elements, shuffled: the chunk boundaries of the scans, the last pack staged in LDS,
the first that is not, and a long one on global memory.

(a) ``merge_rows_packs`` against the op chain it replaces, every output bit for bit."""
import numpy as np
import pytest
import torch

import neus_coarse_ref as cref
import nerf_upsample_ref as ref

pytestmark = pytest.mark.gpu

_CASES = {}


def U():
    from nr3d_lib_amd.bindings import _nerf_upsample
    return _nerf_upsample


def parity_case(m, nc, per_pack):
    """inputs (CPU) and both runs of the restatement, computed once per case and left unchanged"""
    key = (m, nc, per_pack)
    if key not in _CASES:
        depth, sigma, delta, pi, _, _ = ref.soft_shell_packs(ref.parity_lengths(U().LDS_ROW, m, nc))
        P = pi.shape[0]
        u = ref.per_pack_u(P, m) if per_pack else ref.shared_u(m)
        coarse = row = None
        if nc:
            # per-pack cases pick their rows out of a larger table through coarse_row, the others take row p
            coarse = ref.coarse_rows(torch.full((P + 3,), cref.NEAR), torch.linspace(cref.FAR - 0.3, cref.FAR, P + 3), nc)
            row = torch.randperm(P + 3, generator=torch.Generator().manual_seed(7))[:P].contiguous() if per_pack else None
            if row is None:
                coarse = coarse[:P].contiguous()
        kw = dict(coarse=coarse, coarse_row=row)
        _CASES[key] = dict(depth=depth, sigma=sigma, delta=delta, pi=pi, u=u, coarse=coarse, row=row,
                           r32=ref.stage(depth, sigma, delta, pi, u, dtype=torch.float32, **kw),
                           r64=ref.stage(depth, sigma, delta, pi, u, dtype=torch.float64, **kw))
    return _CASES[key]


def _dev(c, dev, *names):
    return [None if c[k] is None else c[k].to(dev) for k in names]


def _check_outputs(fine, merged, deltas, coarse, row, nc, m):
    """what involves no rounding, against the kernel's own new depths"""
    P = fine.shape[0]
    assert (fine.diff(dim=-1) >= 0).all()
    if nc:
        rows = coarse if row is None else coarse[row]
        assert merged.shape == deltas.shape == (P, nc + m)
        assert torch.equal(merged, torch.cat([rows, fine], -1).sort(dim=-1).values)
        assert torch.equal(deltas, torch.cat([merged.diff(dim=-1), torch.zeros_like(merged[:, :1])], -1))
    else:
        assert merged.shape == deltas.shape == (P, m - 1)
        assert torch.equal(deltas, fine.diff(dim=-1)) and torch.equal(merged, fine[:, :m - 1] + fine.diff(dim=-1))


@pytest.mark.parametrize("per_pack", [False, True])
@pytest.mark.parametrize("nc", ref.PARITY_NC)
@pytest.mark.parametrize("m", ref.PARITY_M)
def test_stage_matches_the_restatement(dev, m, nc, per_pack):
    c = parity_case(m, nc, per_pack)
    ref.check_preconditions(c['r64'], c['pi'])
    depth, sigma, delta, pi, u, coarse, row = _dev(c, dev, 'depth', 'sigma', 'delta', 'pi', 'u', 'coarse', 'row')
    fine, merged, deltas = U().upsample_stage_packed(depth, sigma, delta, pi, u, coarse=coarse, coarse_row=row)
    torch.cuda.synchronize()
    assert fine.shape == (pi.shape[0], m) and torch.isfinite(fine).all()
    e_ref = (c['r32']['fine'].double() - c['r64']['fine']).abs().max().item()
    err = (fine.cpu().double() - c['r64']['fine']).abs().max().item()
    allowed = 4 * e_ref + float(np.spacing(np.float32(c['depth'].abs().max().item())))
    print(f"L={U().LDS_ROW} m={m} nc={nc} per_pack={per_pack}: |kernel - f64| {err:.3e}  e_ref {e_ref:.3e}  allowed {allowed:.3e}")
    assert err <= allowed
    one = c['pi'][:, 1] == 1
    assert one.any() and torch.equal(fine.cpu()[one], c['r32']['fine'][one]), "packs of one element"
    _check_outputs(fine, merged, deltas, coarse, row, nc, m)


@pytest.mark.parametrize("nc", ref.PARITY_NC)
def test_packs_without_density_are_exact(dev, nc):
    c = parity_case(9, nc, False)
    depth, sigma, delta, pi, u, coarse = _dev(c, dev, 'depth', 'sigma', 'delta', 'pi', 'u', 'coarse')
    r32 = ref.stage(c['depth'], torch.zeros_like(c['sigma']), c['delta'], c['pi'], c['u'], coarse=c['coarse'], dtype=torch.float32)
    assert (r32['alpha'] == 0).all()
    fine, merged, deltas = U().upsample_stage_packed(depth, torch.zeros_like(sigma), delta, pi, u, coarse=coarse)
    assert torch.equal(fine.cpu(), r32['fine']) and torch.equal(merged.cpu(), r32['merged']) and torch.equal(deltas.cpu(), r32['deltas'])


def test_stage_gives_the_same_bytes_run_after_run(dev):
    c = parity_case(65, 16, True)
    args = _dev(c, dev, 'depth', 'sigma', 'delta', 'pi', 'u')
    coarse, row = _dev(c, dev, 'coarse', 'row')
    first = U().upsample_stage_packed(*args, coarse=coarse, coarse_row=row)
    for _ in range(3):
        again = U().upsample_stage_packed(*args, coarse=coarse, coarse_row=row)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))


def test_stage_without_packs(dev):
    f32 = dict(dtype=torch.float32, device=dev)
    none = torch.empty(0, **f32)
    pi = torch.empty(0, 2, dtype=torch.int64, device=dev)
    fine, merged, deltas = U().upsample_stage_packed(none, none, none, pi, torch.linspace(0.1, 0.9, 9, device=dev))
    assert fine.shape == (0, 9) and merged.shape == deltas.shape == (0, 8)
    fine, merged, deltas = U().upsample_stage_packed(none, none, none, pi, torch.linspace(0.1, 0.9, 9, device=dev),
                                                     coarse=torch.empty(0, 16, **f32))
    assert fine.shape == (0, 9) and merged.shape == deltas.shape == (0, 25)
    # one new depth and no coarse row: there is no interval to return
    depth = torch.tensor([1.0, 2.0, 3.0], **f32)
    fine, merged, deltas = U().upsample_stage_packed(depth, torch.ones(3, **f32), torch.tensor([1.0, 1.0, 0.0], **f32),
                                                     torch.tensor([[0, 3]], device=dev), torch.tensor([0.5], **f32))
    assert fine.shape == (1, 1) and merged.shape == deltas.shape == (1, 0) and 1.0 <= fine.item() <= 3.0


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------

def _merge_inputs(dev, nc=16):
    """rays with and without a marched pack -- the first and the last without --, packs of 1, 63, 64, 65 and L + 3, and marched depths
    that equal coarse ones (one of them twice)"""
    L = U().LDS_ROW
    lens = torch.tensor([0, 1, 63, 0, 64, 65, 0, 0, L + 3, 5, L - nc, L - nc + 1, 0], dtype=torch.int64)
    R = lens.numel()
    pi_all = torch.stack([torch.cumsum(lens, 0) - lens, lens], -1)
    rays = cref.fan_rays(4)
    coarse = ref.coarse_rows(rays['near'][:R], rays['far'][:R], nc)
    which = torch.repeat_interleave(torch.arange(R), lens)
    k = (torch.arange(int(lens.sum())) - pi_all[which, 0]).float()
    depth = (1.7 + 1.5 * k / (lens - 1).clamp_min(1).float()[which]).float()
    b4, b8 = int(pi_all[4, 0]), int(pi_all[8, 0] + pi_all[8, 1])
    below = coarse[4][coarse[4] < depth[b4 + 3]]
    depth[b4:b4 + 3] = torch.stack([below[-2], below[-1], below[-1]])
    depth[b8 - 2:b8] = coarse[8][-1]
    return [t.contiguous().to(dev) for t in (coarse, depth, pi_all, rays['rays_o'][:R], rays['rays_d'][:R])]


def _merge_chain(coarse, depth, pi_all, rays_o, rays_d):
    """the op chain of the driver's first merge"""
    from nr3d_lib_amd.graphics.pack_ops import get_pack_infos_from_batch, merge_two_packs_sorted_a_includes_b, packed_diff
    R, nc = coarse.shape
    dev = coarse.device
    all_rays = torch.arange(R, device=dev)
    hit = pi_all[:, 1].nonzero()[:, 0]
    pidx0, pidx1, pack_infos = merge_two_packs_sorted_a_includes_b(
        coarse.flatten(), get_pack_infos_from_batch(R, nc, device=dev), all_rays, depth, pi_all[hit].contiguous(), hit, b_sorted=True)
    n = depth.numel() + coarse.numel()
    depths_all, ridx_all = depth.new_zeros([n]), hit.new_zeros([n])
    ridx_all[pidx0], ridx_all[pidx1] = all_rays.unsqueeze(-1).expand(-1, nc).flatten(), torch.repeat_interleave(all_rays, pi_all[:, 1])
    depths_all[pidx0], depths_all[pidx1] = coarse.flatten(), depth
    samples_all = torch.addcmul(rays_o[ridx_all], rays_d[ridx_all], depths_all.unsqueeze(-1))
    return depths_all, packed_diff(depths_all, pack_infos), ridx_all, samples_all, pack_infos


def test_merge_equals_the_op_chain_bit_for_bit(dev):
    args = _merge_inputs(dev)
    got, want = U().merge_rows_packs(*args), _merge_chain(*args)
    for name, a, b in zip(("depths_all", "deltas_all", "ridx_all", "samples_all", "pack_infos_out"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} elements differ"
    t, pinfo = got[0].cpu(), got[4].cpu()
    first, n = pinfo[4].tolist()
    assert (t[first:first + n].diff() == 0).sum() >= 3, "the ties are there"
    # and the restatement, which the CPU test pins to the oracle's merge
    r = ref.merge(*[a.cpu() for a in args])
    assert torch.equal(t, r['depths_all']) and torch.equal(got[1].cpu(), r['deltas_all']) and torch.equal(got[2].cpu(), r['ridx_all'])
    assert torch.equal(pinfo, r['pack_infos_out'])
    again = U().merge_rows_packs(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "the same bytes run after run"


def test_merge_with_no_marched_sample_and_with_no_ray(dev):
    coarse, depth, pi_all, o, v = _merge_inputs(dev)
    R, nc = coarse.shape
    none = torch.zeros(R, 2, dtype=torch.int64, device=dev)
    d, dl, ridx, x, pinfo = U().merge_rows_packs(coarse, depth[:0].contiguous(), none, o, v)
    assert torch.equal(d.view(R, nc), coarse) and torch.equal(ridx.view(R, nc), torch.arange(R, device=dev)[:, None].expand(R, nc))
    assert torch.equal(dl.view(R, nc), torch.cat([coarse.diff(dim=-1), torch.zeros_like(coarse[:, :1])], -1))
    assert torch.equal(x, torch.addcmul(o[ridx], v[ridx], d[:, None])) and torch.equal(pinfo[:, 1], torch.full_like(pinfo[:, 1], nc))
    outs = U().merge_rows_packs(coarse[:0].contiguous(), depth[:0].contiguous(), none[:0].contiguous(), o[:0].contiguous(), v[:0].contiguous())
    assert [tuple(t.shape) for t in outs] == [(0,), (0,), (0,), (0, 3), (0, 2)]


def test_argument_checks(dev):
    c = parity_case(9, 16, False)
    depth, sigma, delta, pi, u, coarse = _dev(c, dev, 'depth', 'sigma', 'delta', 'pi', 'u', 'coarse')
    stage = U().upsample_stage_packed
    with pytest.raises(RuntimeError, match="GPU only"):
        stage(depth.cpu(), sigma, delta, pi, u)
    with pytest.raises(RuntimeError, match="`sigma` must be float32"):
        stage(depth, sigma.double(), delta, pi, u)
    with pytest.raises(RuntimeError, match="`delta` must be"):
        stage(depth, sigma, delta[:-1], pi, u)
    with pytest.raises(RuntimeError, match="`pack_infos` must be int64"):
        stage(depth, sigma, delta, pi.int(), u)
    with pytest.raises(RuntimeError, match=r"`pack_infos` must be \[P, 2\]"):
        stage(depth, sigma, delta, pi.flatten(), u)
    with pytest.raises(RuntimeError, match="`u` must be"):
        stage(depth, sigma, delta, pi, u.expand(3, 9).contiguous())
    with pytest.raises(RuntimeError, match="`depth` must be contiguous"):
        stage(torch.stack([depth, depth], -1)[:, 0], sigma, delta, pi, u)
    with pytest.raises(RuntimeError, match="`coarse_row` without `coarse`"):
        stage(depth, sigma, delta, pi, u, coarse_row=torch.zeros(pi.shape[0], dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="without `coarse_row`"):
        stage(depth, sigma, delta, pi, u, coarse=coarse[:-1].contiguous())
    with pytest.raises(RuntimeError, match="`coarse_row` must be int64"):
        stage(depth, sigma, delta, pi, u, coarse=coarse, coarse_row=torch.zeros(pi.shape[0], dtype=torch.int32, device=dev))
    co, d, pi_all, o, v = _merge_inputs(dev)
    merge = U().merge_rows_packs
    with pytest.raises(RuntimeError, match="GPU only"):
        merge(co, d, pi_all.cpu(), o, v)
    with pytest.raises(RuntimeError, match=r"`coarse` must be \[R, nc\]"):
        merge(co.flatten(), d, pi_all, o, v)
    with pytest.raises(RuntimeError, match="`pack_infos_all` must be"):
        merge(co, d, pi_all[:-1].contiguous(), o, v)
    with pytest.raises(RuntimeError, match="`rays_d` must be float32"):
        merge(co, d, pi_all, o, v.half())
    with pytest.raises(RuntimeError, match="`depth` must be"):
        merge(co, d[:, None], pi_all, o, v)
