"""The input families of the permutohedral table tests (tests/permuto_inputs.py), on the CPU with the restatement alone: they
reach the ties, negative coordinates and `sum` corrections they claim, and the GPU tests' own comparison functions catch a rank
comparison that breaks ties the other way (only on the face family, through dL/dx and dL/d(dL_dy)) and a dropped `sum`
correction (through y).  A mutated restatement stands in for the device result.

Nothing is claimed for the `half` family: flipping the rounding tie `up - elev < elev - down` of the nearest remainder-0 point
changed no row of y, dL/dx or dL/dparam at D = 3, 7 and 20 (the `sum` correction brings either choice to the same simplex), so
no comparison could catch it; the family's rows run as plain coverage."""
import os
import re

import pytest
import torch

import permuto_inputs as I
import permuto_ref as R


def mutant_simplex(tie_le=False, drop_sum=False):
    """R.simplex with `<=` in the rank comparison and / or without the `sum` correction (both False: R.simplex, asserted below)"""
    def simplex(x32, sc32, sh32):
        N, D = x32.shape
        elev = [None] * (D + 1)
        sm = torch.zeros(N, dtype=torch.float32)
        for dim in range(D, 0, -1):
            p = x32[:, dim - 1] + (sh32[dim - 1] if sh32 is not None else torch.tensor(0., dtype=torch.float32))
            cf = p * sc32[dim - 1]
            elev[dim] = sm - cf * torch.tensor(float(dim), dtype=torch.float32)
            sm = sm + cf
        elev[0] = sm
        elev = torch.stack(elev, 1)
        v = elev / torch.tensor(float(D + 1), dtype=torch.float32)
        down = torch.floor(v).to(torch.int64) * (D + 1)
        up = down + (D + 1)
        rem0 = torch.where(up.to(torch.float32) - elev < elev - down.to(torch.float32), up, down)
        s = torch.div(rem0.sum(1), D + 1, rounding_mode='trunc')
        if drop_sum:
            s = torch.zeros_like(s)
        rank = torch.zeros(N, D + 1, dtype=torch.int64)
        diff = elev - rem0.to(torch.float32)
        for dim in range(D):
            for o in range(dim + 1, D + 1):
                c = (diff[:, dim] <= diff[:, o]) if tie_le else (diff[:, dim] < diff[:, o])
                rank[:, dim] += c.long()
                rank[:, o] += (~c).long()
        rank = rank + s[:, None]
        lo, hi = rank < 0, rank > D
        rank = torch.where(lo, rank + D + 1, torch.where(hi, rank - D - 1, rank))
        rem0 = torch.where(lo, rem0 + D + 1, torch.where(hi, rem0 - D - 1, rem0))
        return elev, rem0, rank
    return simplex


def _simplices(D, family):
    """R.simplex of the family's points at both levels -> list of (elev, rem0 before the correction, sum, rank)"""
    c = I.case(D, 2, family)
    sc = I.scales_of(c["meta"])
    out = []
    for lvl in range(len(I.RES)):
        sh = c["shifts"][lvl] if c["shifts"] is not None else None
        elev, rem0, rank = R.simplex(c["x"], sc[lvl], sh)
        down = torch.floor(elev / torch.tensor(float(D + 1))).to(torch.int64) * (D + 1)
        up = down + (D + 1)
        near = torch.where(up.float() - elev < elev - down.float(), up, down)
        out.append(dict(elev=elev, down=down, up=up, near=near, sum=torch.div(near.sum(1), D + 1, rounding_mode='trunc'), rank=rank))
    return out


def _dims_of(family):
    return R.SUPPORTED if family in ("wide", "table") else I.FACE_DIMS


@pytest.mark.parametrize("family", I.FAMILIES)
def test_rank_is_a_permutation(family):
    for D in _dims_of(family):
        for s in _simplices(D, family):
            assert torch.equal(s["rank"].sort(1).values, torch.arange(D + 1).expand(I.N, D + 1)), (family, D)


def test_unmutated_copy_is_the_restatement():
    c = I.case(7, 2, "table")
    sc = I.scales_of(c["meta"])
    for a, b in zip(R.simplex(c["x"], sc[1], c["shifts"][1]), mutant_simplex()(c["x"], sc[1], c["shifts"][1])):
        assert torch.equal(a, b)


def test_face_family_ties():
    """share of (row, level) pairs with at least two equal `elev - rem0`: >= 0.25 at every D, >= 0.9 from D = 7"""
    assert (I.case(3, 2, "face")["x"] == 0).all(1).sum() == I.N // 4          # the origin itself
    for D in I.FACE_DIMS:
        c = I.case(D, 2, "face")
        nz = (c["x"] != 0).sum(1)
        assert torch.equal(nz, (torch.arange(I.N) % 4).clamp(max=D)) and c["x"].abs().max() < 3
        two = nz >= 2
        eq = torch.tensor([len(set(row[row != 0].tolist())) < int(k) for row, k in zip(c["x"], nz)])
        assert abs(int((eq & two).sum()) * 2 - int(two.sum())) <= 2            # two equal coordinates in half of them
        tied = []
        for s in _simplices(D, "face"):
            diff = s["elev"] - s["near"].float()
            tied.append(torch.tensor([len(set(row.tolist())) <= D for row in diff]))
        share = float(torch.stack(tied).float().mean())
        print(f"face D={D}: tie share {share:.2f}")
        assert share >= (0.9 if D >= 7 else 0.25), (D, share)


def test_half_family_reaches_the_rounding_tie():
    for D in I.FACE_DIMS:
        hit = 0
        for s in _simplices(D, "half"):
            e = s["elev"]
            hit += int(((s["up"].float() - e == e - s["down"].float()).any(1)).sum())
        print(f"half D={D}: {hit} (row, level) pairs on the rounding tie")
        assert hit >= 1, D


def test_wide_family_goes_below_zero_and_off_the_plane():
    for D in R.SUPPORTED:
        ss = _simplices(D, "wide")
        assert any(bool((s["elev"] < 0).any()) for s in ss), D
        assert any(bool((s["sum"] != 0).any()) for s in ss), D


def _mutated(D, family, **flags):
    c = I.case(D, 2, family)
    with I.simplex_replaced(mutant_simplex(**flags)):
        return I.compute_reference(c["meta"], c["x"], c["p"], c["gy"], c["ggx"], c["shifts"])


@pytest.mark.parametrize("D", I.FACE_DIMS)
def test_teeth_rank_tie_broken_the_other_way(D):
    """`<=` for the reference's strict `<`: caught on the face family through dL/dx (and dL/d(dL_dy)), at both dtypes' bounds,
    while y and dL/dparam stay (continuity, zero weights); not caught by anything on random points -- why the family exists"""
    want, lv = I.reference(D, 2, "face"), I.case(D, 2, "face")["levels"]
    got = _mutated(D, "face", tie_le=True)
    for dt in I.DTYPES:
        I.compare("y", got["y"], want["y"], dt, lv)
        I.compare("dL_dparam", got["dL_dparam"], want["dL_dparam"], dt, lv)
        with pytest.raises(AssertionError, match="dL_dx"):
            I.compare("dL_dx", got["dL_dx"], want["dL_dx"], dt, lv)
        with pytest.raises(AssertionError, match="dL_ddLdy"):
            I.compare("dL_ddLdy", got["dL_ddLdy"], want["dL_ddLdy"], dt, lv)
    I.compare_all(_mutated(D, "table", tie_le=True), I.reference(D, 2, "table"), torch.float32, I.case(D, 2, "table")["levels"])


@pytest.mark.parametrize("D", I.FACE_DIMS)
@pytest.mark.parametrize("family", I.FAMILIES)
def test_teeth_dropped_sum_correction(D, family):
    """without the `sum` correction a point whose nearest remainder-0 point is off the plane lands in a wrong simplex: caught
    through y on every family"""
    got = _mutated(D, family, drop_sum=True)
    for dt in I.DTYPES:
        with pytest.raises(AssertionError, match="y "):
            I.compare("y", got["y"], I.reference(D, 2, family)["y"], dt)


def test_table_cases_cover_every_compiled_kernel():
    """the NR3D_PERMUTO_CASE(..) numbers of csrc/permuto_d*.hip are exactly the supported dimensions, each once; the
    every-table-entry test is parametrised over all of them x 2 widths x 2 dtypes and launches four kernels per case"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nr3d_lib_amd", "csrc")
    found = []
    for f in sorted(os.listdir(src)):
        if re.fullmatch(r"permuto_d[a-z]\.hip", f):
            with open(os.path.join(src, f)) as fh:
                found += [int(v) for v in re.findall(r"NR3D_PERMUTO_CASE\((\d+)\)", fh.read())]
    assert sorted(found) == R.SUPPORTED and len(set(found)) == len(found)
    assert sorted(set(I.TABLE_CASES), key=str) == sorted(I.TABLE_CASES, key=str)
    assert {(D, w) for D, w, _ in I.TABLE_CASES} == {(D, w) for D in found for w in (2, 4)}
    n_kernels = 4 * len(I.TABLE_CASES)       # forward, dL/dx, dL/dparam, double backward
    print(f"{n_kernels} kernels launched by the every-table-entry test")
    assert n_kernels == 432
