"""The decision inputs of the up-sampling stages (tests/upsample_decision_inputs.py) without a GPU.

1. Every family meets its own conditions on the float64 run (asserted where it is built), and the per-pack condition on the yardstick:
   no pack's allowed error exceeds 1e-3 (far - near).  The margins are printed.
2. The restatements are right on these inputs: the packed NeuS and NeRF restatements against the CPU oracle's pack-op chain (`fine`
   within one ulp, positions exact), as tests/test_neus_packed_cpu.py and tests/test_nerf_upsample_cpu.py do on the sphere and the
   shell; the row restatement against the torch helpers that tests/test_neus_coarse_cpu.py pins to the reference's results, under that
   file's tolerances.
3. The inputs can tell wrong kernels apart, which is the proof that tests/test_upsample_decisions_gpu.py can fail.  A mutant is the
   float32 restatement with ONE constant moved by a factor 10 (the slope clamp to -1 and -100), or with one rule replaced: below the
   pmf floor the lerp instead of the bin's lower depth (packs) or of den = 1 (rows), and the early stop honoured in the first chunk of
   64 elements only.  Every mutant must leave the float64 run of the TRUE restatement by at least 10 x the allowed error in at
   least one pack of one family: the kernel itself may sit at 1 x allowed, and a mutant at 2 x could hide behind association noise.
   A result that is not finite counts as infinitely far (the GPU test asserts finiteness).
4. The same mutants on the parity inputs of the existing value tests, under their whole-call yardstick: a printed table, no assertion.
   It is the gap this file closes."""
import numpy as np
import pytest
import torch

import nerf_upsample_ref as nref
import neus_coarse_ref as cref
import neus_packed_ref as pref
import upsample_decision_inputs as D

L = 512                 # the LDS row the library is built with by default; the GPU file asks the library
SEPARATION = 10.0


def _show(name, key, c):
    print(f"{name}{key}: " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in c['margins'].items()))


# ---- 1. the families' own conditions ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", D.PACKED_FAMILIES)
def test_families_meet_their_conditions(family):
    for est in D.estimates_of(family):
        c = D.packed_case(family, L, est)
        _show("packed", (family, est), c)
        assert c['allowed'].max().item() <= D.SPAN_TOL
        assert (c['pi'][:, 1] - (D.M if family == 'second' else 0)).tolist() == D.packed_lengths(L, D.M)
        for R, n in D.ROW_SHAPES:
            r = D.rows_case(family, R, n, est)
            _show("rows", (family, R, n, est), r)
            assert r['allowed'].max().item() <= D.SPAN_TOL and r['depth'].shape == (R, n)
    if family in D.NERF_FAMILIES:
        for nc in nref.PARITY_NC:
            c = D.nerf_case(family, L, nc)
            _show("nerf", (family, nc), c)
            assert c['allowed'].max().item() <= D.SPAN_TOL
    if family in D.INVERT_FAMILIES:
        c = D.invert_case(family, L)
        _show("invert", (family,), c)
        assert c['allowed'].max().item() <= D.SPAN_TOL


@pytest.mark.parametrize("lds_row", [256, 1024])
def test_families_hold_for_the_other_lds_rows(lds_row):
    """the library can be built with an LDS row of 256, 512 or 1024 elements; the longest pack follows it"""
    for family in D.PACKED_FAMILIES:
        for est in D.estimates_of(family):
            assert D.packed_case(family, lds_row, est)['allowed'].max().item() <= D.SPAN_TOL
    for family in D.NERF_FAMILIES:
        for nc in nref.PARITY_NC:
            assert D.nerf_case(family, lds_row, nc)['allowed'].max().item() <= D.SPAN_TOL


# ---- 2. the restatements on the new inputs ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", D.PACKED_FAMILIES)
def test_packed_restatement_matches_oracle_chain(oracle, family):
    for est in D.estimates_of(family):
        c = D.packed_case(family, L, est)
        depth, pi, u, r = c['depth'], c['pi'], c['u'], c['r32']
        m = u.shape[1]
        alpha, pinfo = r['alpha'].numpy(), pi.numpy()
        w = oracle.packed_alpha_to_vw_forward(alpha, pinfo, 1e-4, 0.0, False)[0]
        cdf = np.zeros_like(w)
        for b, n in pinfo:
            cs = np.concatenate([[0], np.cumsum(w[b:b + n - 1], dtype=np.float32)]).astype(np.float32)
            cdf[b:b + n] = cs / max(cs[-1], np.float32(1e-5))
        fine = oracle.packed_invert_cdf(depth.numpy(), cdf, np.ascontiguousarray(u.numpy()), pinfo)[0]
        fine = np.maximum.accumulate(fine, axis=-1)          # the stage raises a row to its running maximum: one rounding of the fma at most
        ulp = np.spacing(np.abs(fine).astype(np.float32))
        assert (np.abs(fine.astype(np.float64) - r['fine'].double().numpy()) <= ulp).all(), (family, est)
        lb = [torch.searchsorted(depth[b:b + n].contiguous(), torch.from_numpy(fine[p]).contiguous()) for p, (b, n) in enumerate(pinfo)]
        pinfo_fine = np.stack([np.arange(len(pinfo)) * m, np.full(len(pinfo), m)], 1).astype(np.int64)
        pa, pb, pim = oracle.try_merge_two_packs_sorted_aligned(depth.numpy(), pinfo, fine.ravel(), pinfo_fine, b_sorted=True)
        for p, (b, n) in enumerate(pinfo):
            start, old, new = pref.merge_positions(int(b), int(n), lb[p], p)
            assert (start, n + m) == tuple(pim[p])
            np.testing.assert_array_equal(pa[b:b + n], old.numpy())
            np.testing.assert_array_equal(pb[p * m:(p + 1) * m], new.numpy())


@pytest.mark.parametrize("family", D.NERF_FAMILIES)
def test_nerf_restatement_matches_oracle_chain(oracle, family):
    c = D.nerf_case(family, L, 16)
    depth, pi, u, r = c['depth'], c['pi'], c['u'], c['r32']
    P, m = u.shape
    alpha, pinfo = r['alpha'].numpy(), pi.numpy()
    cs = oracle.packed_cumsum(alpha, pinfo)
    last = cs[pinfo[:, 0] + pinfo[:, 1] - 1]
    cdf = (cs / np.repeat(np.maximum(last, np.float32(1e-5)), pinfo[:, 1])).astype(np.float32)
    mask = nref.padded(pi, depth.shape[0])[1]
    np.testing.assert_array_equal(cdf, r['cdf'][mask].numpy())
    fine, bins = oracle.packed_invert_cdf(depth.numpy(), cdf, np.ascontiguousarray(u.numpy()), pinfo)
    np.testing.assert_array_equal(bins, (pi[:, :1] + r['pos']).numpy())
    fine = np.maximum.accumulate(fine, axis=-1)
    ulp = np.spacing(np.abs(fine).astype(np.float32))
    assert (np.abs(fine.astype(np.float64) - r['fine'].double().numpy()) <= ulp).all()
    # the union with the coarse rows on the restatement's own new depths: positions and differences exactly
    own, rows = r['fine'].numpy(), c['coarse'][c['row']].numpy()
    nc = rows.shape[1]
    pinfo_c = np.stack([np.arange(P) * nc, np.full(P, nc)], 1).astype(np.int64)
    pinfo_f = np.stack([np.arange(P) * m, np.full(P, m)], 1).astype(np.int64)
    pa, pb, pim = oracle.try_merge_two_packs_sorted_aligned(rows.ravel(), pinfo_c, own.ravel(), pinfo_f, b_sorted=True)
    begin = (torch.arange(P) * (nc + m))[:, None]
    np.testing.assert_array_equal(pa.reshape(P, nc), (begin + r['pos_coarse']).numpy())
    np.testing.assert_array_equal(pb.reshape(P, m), (begin + r['pos_fine']).numpy())
    merged = np.empty(P * (nc + m), np.float32)
    merged[pa], merged[pb] = rows.ravel(), own.ravel()
    np.testing.assert_array_equal(merged.reshape(P, nc + m), r['merged'].numpy())
    np.testing.assert_array_equal(oracle.packed_diff(merged, pim).reshape(P, nc + m), r['deltas'].numpy())


@pytest.mark.parametrize("family", D.PACKED_FAMILIES)
def test_row_restatement_matches_the_torch_helpers(family):
    """the helpers sample at the shared row of CDF positions, so that is what both sides invert here; the family's own u rows
    differ from it in where they look, not in what is looked at"""
    from test_neus_coarse_cpu import ALPHA_TOL, SAMPLE_TOL
    from nr3d_lib_amd.graphics import raysample as rs
    from nr3d_lib_amd.graphics.nerf.nerf_utils import ray_alpha_to_vw
    from nr3d_lib_amd.graphics.neus import neus_utils as nu
    for est in D.estimates_of(family):
        for R, n in D.ROW_SHAPES:
            c = D.rows_case(family, R, n, est)
            d, s, inv_s = c['depth'], c['sdf'], c['inv_s']
            alpha = nu.neus_ray_sdf_to_upsample_alpha(s, d, inv_s) if est else nu.neus_ray_sdf_to_alpha(s, inv_s, fused=False)
            w = ray_alpha_to_vw(alpha)
            r = cref.stage(d, s, cref.shared_u(D.M), inv_s, est, torch.float32)
            cdf = torch.cat([torch.zeros(R, 1), torch.cumsum(w / w.sum(-1, keepdim=True).clamp_min(1e-5), -1)], -1)
            assert (cdf.double() - r['cdf'].double()).abs().max().item() <= ALPHA_TOL * n, (family, R, n, est)
            got = rs.batch_sample_pdf(d, w, D.M)
            agree = (got.double() - r['fine'].double()).abs() <= SAMPLE_TOL
            # where the two differ by more, a CDF value lies within the CDF's own tolerance of the position: another bin, not another rule
            near = ((r['cdf'].double()[:, None, :] - cref.shared_u(D.M).double()[None, :, None]).abs().amin(-1) <= ALPHA_TOL * n)
            assert (agree | near).all() and agree.float().mean().item() > 0.98, (family, R, n, est, agree.float().mean().item())


# ---- 3. and 4. mutants ----------------------------------------------------------------------------------------------------------------

ROWS_MUTANTS = {
    'slope clamp -1': dict(slope_clamp=-1.0), 'slope clamp -100': dict(slope_clamp=-100.0),
    'mass floor 1e-6': dict(mass_min=1e-6), 'mass floor 1e-4': dict(mass_min=1e-4),
    'den floor 1e-6': dict(den_min=1e-6), 'den floor 1e-4': dict(den_min=1e-4),
    'alpha eps 1e-6': dict(alpha_eps=1e-6), 'alpha eps 1e-4': dict(alpha_eps=1e-4),
    'slope eps 1e-6': dict(slope_eps=1e-6), 'slope eps 1e-4': dict(slope_eps=1e-4),
    'lerp below the floor': dict(den_min=0.0),
}
PACKED_MUTANTS = {
    'slope clamp -1': dict(SLOPE_CLAMP=-1.0), 'slope clamp -100': dict(SLOPE_CLAMP=-100.0),
    'mass floor 1e-6': dict(MASS_MIN=1e-6), 'mass floor 1e-4': dict(MASS_MIN=1e-4),
    'pmf floor 1e-6': dict(PMF_MIN=1e-6), 'pmf floor 1e-4': dict(PMF_MIN=1e-4),
    'early stop 1e-5': dict(EARLY_STOP=1e-5), 'early stop 1e-3': dict(EARLY_STOP=1e-3),
    'alpha eps 1e-6': dict(ALPHA_EPS=1e-6), 'alpha eps 1e-4': dict(ALPHA_EPS=1e-4),
    'slope eps 1e-6': dict(SLOPE_EPS=1e-6), 'slope eps 1e-4': dict(SLOPE_EPS=1e-4),
    'lerp below the floor': dict(PMF_MIN=0.0), 'stop in the first chunk only': dict(STOP_FIRST_CHUNK_ONLY=True),
}
NERF_MUTANTS = {
    'mass floor 1e-6': dict(MASS_MIN=1e-6), 'mass floor 1e-4': dict(MASS_MIN=1e-4),
    'pmf floor 1e-6': dict(PMF_MIN=1e-6), 'pmf floor 1e-4': dict(PMF_MIN=1e-4), 'lerp below the floor': dict(PMF_MIN=0.0),
}
INVERT_MUTANTS = {k: v for k, v in NERF_MUTANTS.items() if 'PMF_MIN' in v}
ESTIMATE_ONLY = ('slope clamp', 'slope eps')


def decision_cases(kind):
    """(label, case) of every decision input of one stage"""
    if kind == 'rows':
        return [((f, R, n, est), D.rows_case(f, R, n, est)) for f in D.PACKED_FAMILIES for est in D.estimates_of(f) for R, n in D.ROW_SHAPES]
    if kind == 'packed':
        return [((f, est), D.packed_case(f, L, est)) for f in D.PACKED_FAMILIES for est in D.estimates_of(f)]
    if kind == 'nerf':
        return [((f, nc), D.nerf_case(f, L, nc)) for f in D.NERF_FAMILIES for nc in nref.PARITY_NC]
    return [((f,), D.invert_case(f, L)) for f in D.INVERT_FAMILIES]


def best_ratio(kind, constants, cases, name):
    """the largest (mutant's distance to the float64 run) / (allowed error) over the packs of the cases -> (ratio, label)"""
    best, where = 0.0, None
    with np.errstate(all='ignore'):
        for label, c in cases:
            if name.startswith(ESTIMATE_ONLY) and not c.get('est', False):
                continue
            fine = D.RUNNERS[kind](c, torch.float32, **constants)['fine']
            ratio = (D.per_pack_error(fine, c['r64']['fine']) / c['allowed']).max().item()
            if ratio > best:
                best, where = ratio, label
    return best, where


@pytest.mark.parametrize("kind,mutants", [('rows', ROWS_MUTANTS), ('packed', PACKED_MUTANTS), ('nerf', NERF_MUTANTS), ('invert', INVERT_MUTANTS)])
def test_every_mutant_is_told_apart(kind, mutants):
    cases = decision_cases(kind)
    true_ratio, _ = best_ratio(kind, {}, cases, '')
    print(f"{kind}: the true float32 restatement sits at {true_ratio:.2f} x allowed (4 e_ref + ulp: at most 0.25 + the ulp's share)")
    assert true_ratio <= 1.0
    missed = []
    for name, constants in mutants.items():
        ratio, where = best_ratio(kind, constants, cases, name)
        print(f"{kind:7s} {name:30s} {ratio:12.4g} x allowed  at {where}")
        if not ratio >= SEPARATION:
            missed.append((name, ratio))
    assert not missed, f"{kind}: mutants within {SEPARATION} x allowed on every input: {missed}"


def parity_cases(kind):
    """inputs of the existing value tests, with the whole-call yardstick they are compared under: every pack gets the call's allowance"""
    out = []
    if kind == 'rows':
        for n, m in ((17, 9), (65, 65)):
            for est in (False, True):
                R = 64
                rays = cref.fan_rays(8)
                o, v = rays['rays_o'][:R], rays['rays_d'][:R]
                depth = torch.linspace(cref.NEAR, cref.FAR, n).expand(R, n).contiguous()
                sdf = ((o[:, None, :] + v[:, None, :] * depth[..., None]).norm(dim=-1) - cref.RADIUS).contiguous()
                out.append(((n, m, est), dict(depth=depth, sdf=sdf, u=cref.shared_u(m), inv_s=64.0, est=est)))
    elif kind == 'packed':
        for m in (9, 65):
            for est in (False, True):
                depth, sdf, pi = pref.sphere_packs(pref.parity_lengths(L, m))
                out.append(((m, est), dict(depth=depth, sdf=sdf, pi=pi, u=cref.shared_u(m), inv_s=64.0, est=est)))
    else:
        for m in (9, 65):
            depth, sigma, delta, pi, _, _ = nref.soft_shell_packs(nref.parity_lengths(L, m, 0))
            c = dict(depth=depth, sigma=sigma, delta=delta, pi=pi, u=nref.per_pack_u(pi.shape[0], m))
            if kind == 'invert':
                mask = nref.padded(pi, depth.shape[0])[1]
                c['cdf'] = nref.stage(depth, sigma, delta, pi, c['u'], dtype=torch.float32)['cdf'][mask].contiguous()
            out.append(((m,), c))
    for _, c in out:
        r32, r64 = D.RUNNERS[kind](c, torch.float32), D.RUNNERS[kind](c, torch.float64)
        c['r64'] = r64
        c['allowed'] = torch.full((r64['fine'].shape[0],), D.allowed_error(r32['fine'], r64['fine'], c['depth']).max().item())
    return out


def test_the_gap_on_the_parity_inputs():
    """printed, not asserted: most mutants stay inside the allowed error of the value tests' own inputs"""
    for kind, mutants in (('rows', ROWS_MUTANTS), ('packed', PACKED_MUTANTS), ('nerf', NERF_MUTANTS), ('invert', INVERT_MUTANTS)):
        cases = parity_cases(kind)
        for name, constants in mutants.items():
            ratio, where = best_ratio(kind, constants, cases, name)
            print(f"parity {kind:7s} {name:30s} {ratio:12.4g} x allowed  {'noticed' if ratio > 1 else 'NOT noticed'}")
