"""GPU: the one packed up-sampling loop of the NeuS march-occ drivers (graphics.neus._packed_upsample.upsample_loop) called with and
without labels on the same packs -- the parity packs of tests/test_neus_upsample_packed_gpu.py, lengths 1 .. 2 L + 7 shuffled so
that LDS and global packs share workgroups and the last workgroup is partial, on the analytic sphere of neus_coarse_ref.

Per route the two calls run the same kernel body (fused) or the same ops (chain) on the same numbers, so every depth is compared
with torch.equal.  The labels are judged against the loop's own unions restated on the host: an old element keeps its label, a new
one carries the label the loop returned for it."""
import pytest
import torch

import neus_coarse_ref as cref
import neus_forest_ref as fref
import neus_packed_ref as ref

pytestmark = pytest.mark.gpu

M = 9
_INPUTS = {}


def inputs(dev):
    """built once and left unchanged: (o, d of every pack, depth, sdf, pack_infos, labels) on the device"""
    if "in" not in _INPUTS:
        from nr3d_lib_amd.bindings import _neus_upsample as U
        depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(U.PACKED_LDS_ROW, M))
        rays = cref.fan_rays(4)
        sel = torch.arange(pi.shape[0]) % 16                                  # sphere_packs takes the rays in turn
        _INPUTS["in"] = tuple(t.to(dev) for t in (rays['rays_o'][sel], rays['rays_d'][sel], depth, sdf, pi, fref.labels_every(pi)))
    return _INPUTS["in"]


def host_union(depth, blidx, pi, fine, blidx_fine):
    """the union of one factor on the host: a new depth before an equal old one (neus_packed_ref.merge_positions)"""
    m = fine.shape[1]
    d_new, b_new = depth.new_empty(depth.numel() + fine.numel()), blidx.new_empty(depth.numel() + fine.numel())
    pi_new = torch.stack([pi[:, 0] + torch.arange(pi.shape[0]) * m, pi[:, 1] + m], -1)
    for p, (b, n) in enumerate(pi.tolist()):
        lb = torch.searchsorted(depth[b:b + n].contiguous(), fine[p].contiguous())
        _, old, new = ref.merge_positions(b, n, lb, p)
        d_new[old], d_new[new] = depth[b:b + n], fine[p]
        b_new[old], b_new[new] = blidx[b:b + n], blidx_fine[p]
    return d_new, b_new, pi_new


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("est", [False, True])
@pytest.mark.parametrize("factors", [[1, 4, 16], [1]])
def test_loop_with_and_without_labels(dev, monkeypatch, factors, est, fused, perturb):
    from nr3d_lib_amd.bindings import _neus_upsample as U
    from nr3d_lib_amd.graphics.neus._packed_upsample import upsample_loop
    o, d, depth, sdf, pi, bl = inputs(dev)
    calls = dict(plain=[], blocks=[])
    for key, name in (("plain", "upsample_stage_packed"), ("blocks", "upsample_stage_packed_blocks")):
        def counted(*a, merge=True, need_sdf=True, _real=getattr(U, name), _seen=calls[key]):
            _seen.append((merge, need_sdf))
            return _real(*a, merge=merge, need_sdf=need_sdf)
        monkeypatch.setattr(U, name, counted)

    def run(blidx):
        seen = []

        def sdf_at(x, labels):
            assert x.shape[0] == pi.shape[0] and x.shape[1:] == (M, 3)
            assert (labels is None) if blidx is None else (labels.shape == x.shape[:2] and labels.dtype == torch.int64)
            seen.append(labels)
            return x.norm(dim=-1) - cref.RADIUS

        torch.manual_seed(7)
        out = upsample_loop(o, d, depth, sdf, pi.clone(), blidx, [M] * len(factors), factors, 64.0, est, perturb, fused, sdf_at)
        assert len(seen) == len(factors) - 1, "one SDF query between two factors, none behind the last"
        return out

    fines, none, (d_end, b_none, pi_end) = run(None)
    want = [(True, True)] * (len(factors) - 1) + [(False, False)] if fused else []
    assert calls == dict(plain=want, blocks=[])
    fines_l, labels, (d_end_l, b_end, pi_end_l) = run(bl)
    assert calls == dict(plain=want, blocks=want)
    assert none is None and b_none is None and len(fines) == len(fines_l) == len(labels) == len(factors)
    for f, f_l, lab in zip(fines, fines_l, labels):
        assert f.shape == (pi.shape[0], M) and lab.shape == f.shape and lab.dtype == torch.int64
        assert torch.equal(f, f_l)
    assert torch.equal(d_end, d_end_l) and torch.equal(pi_end, pi_end_l)
    # the state the last factor saw: the unions of all factors before it, labels carried along
    d_host, b_host, pi_host = depth.cpu(), bl.cpu(), pi.cpu()
    for f, lab in zip(fines_l[:-1], labels[:-1]):
        d_host, b_host, pi_host = host_union(d_host, b_host, pi_host, f.cpu(), lab.cpu())
    assert torch.equal(pi_end.cpu(), pi_host) and torch.equal(d_end.cpu(), d_host)
    assert torch.equal(b_end.cpu(), b_host), "an old element keeps its label, a new one has the label the loop returned for it"
