"""Non-finite and extreme gradients on every dL/dparam route (and the dL/dx, Hessian and forward kernels).

Contract, per route: the output of a call with NaN / +-inf in a few chosen VALUES (dL/dy, dL/d(dL/dx), table entries -- never
x: a non-finite position is a table index) against the oracle on the same inputs (`accum_double=True`):
  (a) isfinite(got) == isfinite(want), element for element -- no laundering (a non-finite update turned into a finite
      number, e.g. by a fixed-point conversion) and no leaking (non-finite values in entries the row does not touch);
      NaN and inf count the same, as they do for a GradScaler;
  (b) the finite entries within the usual tolerance of the oracle.
Most routes accumulate dL/dparam in 64-bit fixed point with a scale from a bound they compute themselves and fall back to
fp64 when that bound is not finite ("Non-finite gradients"); a bound that lets a NaN through keeps the fixed
point on and fails (a).  The second half of the file checks the scales at the edges of the magnitude range."""
import itertools

import numpy as np
import pytest
import torch

from util import LOTD_CASES, REL_TOL, assert_close, lotd_inputs

pytestmark = pytest.mark.gpu

N = 60013
HALF_TOL = 1e-3       # one rounding to half (the LoTD half tests' bound)
C2_N = 1 << 20


def _np64(a):
    return (a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def check(got, want, name, levels=None, rel=REL_TOL, some_nonfinite=True):
    """(a) the same non-finite mask as the oracle, (b) the finite entries within `rel` (per level / per column)"""
    got, want = _np64(got), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{name}: shape {got.shape} vs {want.shape}"
    fg, fw = np.isfinite(got), np.isfinite(want)
    if some_nonfinite:
        assert not fw.all(), f"{name}: the oracle has no non-finite entry (the test input does not reach the case)"
    if not np.array_equal(fg, fw):
        laundered, leaked = np.argwhere(fg & ~fw), np.argwhere(~fg & fw)
        raise AssertionError(f"{name}: {len(laundered)} entries finite where the oracle's are not (first "
                             f"{laundered[:3].tolist()}: {[got[tuple(i)] for i in laundered[:3]]}), {len(leaked)} non-finite "
                             f"where the oracle's are finite (first {leaked[:3].tolist()})")
    assert_close(np.where(fw, got, 0.0), np.where(fw, want, 0.0), rel=rel, name=name, levels=levels)


def _metas(oracle, case):
    from nr3d_lib_amd.bindings import _lotd
    if case == "c2":
        from nr3d_lib_amd.models.grid_encodings.lotd import gen_ngp_cfg
        cfg = gen_ngp_cfg()
        args = (3, cfg["lod_res"], cfg["lod_n_feats"], cfg["lod_types"], cfg["hashmap_size"], False)
    elif case == "lds_stage":           # test_lotd_gpu.py test_forward_lds_stage_bit_identical's meta
        args = (3, [16, 22, 30, 42, [36, 20, 50], 58, 111, 212], [2] * 8, ["Dense"] * 6 + ["Hash"] * 2, 2 ** 16, False)
    else:
        args = LOTD_CASES[case]
    return _lotd, oracle.lotd_create_meta(*args), _lotd.LoDMeta(*args)


@pytest.fixture(scope="module")
def inputs(oracle):
    """inputs(case, n=None, seed=0) -> (_lotd, oracle meta, meta, (x, params, dL_dy, dL_ddLdx), per-set cache dict), built once
    per (case, n, seed) and shared by the tests of this file (the C2 set at 2^20 points); freed when the file is done"""
    store = {}

    def get(case, n=None, seed=0):
        n = n or (C2_N if case == "c2" else N)
        key = (case, n, seed)
        if key not in store:
            _lotd, m_ref, m = _metas(oracle, case)
            store[key] = (_lotd, m_ref, m, lotd_inputs(m_ref.as_dict(), n, seed), {})
        return store[key]

    yield get
    store.clear()


def _rows(n):
    return [3, n // 3, n - 2]


def poison(a, kind, n_cols, n):
    """a copy of `a` [n, n_cols] with non-finite values in three rows: 'nan1' NaN in ONE feature of a pseudo level (the other
    feature finite) of the first, a middle and the last pseudo level; 'inf1' the same with +inf / -inf / +inf; 'nan2' NaN in both
    features of a pseudo level in one row and in one feature of another row"""
    a = a.copy()
    r = _rows(n)
    last, mid = n_cols - 1, 2 * ((n_cols // 2) // 2) + 1
    if kind == "nan1":
        a[r[0], 0] = a[r[1], mid] = a[r[2], last] = np.nan
    elif kind == "inf1":
        a[r[0], 0], a[r[1], mid], a[r[2], last] = np.inf, -np.inf, np.inf
    elif kind == "nan2":
        a[r[0], 0:2] = np.nan
        a[r[1], mid] = np.nan
    else:
        raise ValueError(kind)
    return a


def _oracle_dx(oracle, m_ref, g, x, p, chunk=1 << 16):
    """oracle dL/dx in chunks of points (the [N, E, D] Jacobian of C2 at 2^20 points would be 0.4 GB)"""
    out = []
    for s in range(0, x.shape[0], chunk):
        _, j_ref = oracle.lotd_fwd(m_ref, x[s:s + chunk], p, need_dydx=True)
        out.append(oracle.lotd_bwd_dx(m_ref, g[s:s + chunk], j_ref))
    return np.concatenate(out)


def _t(dev, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


# ---------------------------------------------------------------------------------------------------------------------
# LoTD dL/dparam, first order
# ---------------------------------------------------------------------------------------------------------------------
PAIR_ROUTES = list(itertools.product((1, 0), repeat=4))        # pair_fold, pair_fixed, pair_quad, pair_direct


@pytest.mark.parametrize("case", ["ngp_pair", "pair_f4", "c2"])
@pytest.mark.parametrize("kind", ["nan1", "inf1", "nan2"])
def test_pair_path_dparam(oracle, inputs, dev, hip_option, case, kind):
    """the pair path on every combination of its options (dL/dx in the same call: the folded route takes its scale from the
    dL/dx kernel's per-workgroup slots), with and without dL/dx, and the corner-record route (lotd_pair = 0)"""
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case)
    n = x.shape[0]
    gp = poison(g, kind, m.n_encoded_dims, n)
    xt, pt, gt = _t(dev, x, p, gp)
    want = oracle.lotd_bwd_dparam(m_ref, gp, x, p, accum_double=True)
    want_dx = _oracle_dx(oracle, m_ref, gp, x, p)
    _, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
    for fold, fixed, quad, direct in PAIR_ROUTES:
        for k, val in (("pair_fold", fold), ("pair_fixed", fixed), ("pair_quad", quad), ("pair_direct", direct)):
            hip_option(k, val)
        dx, dp = _lotd.lod_bwd(m, gt, xt, pt, j, need_input_grad=True, need_param_grad=True)
        tag = f"fold={fold} fixed={fixed} quad={quad} direct={direct}"
        check(dp, want, f"dL/dparam ({tag})", levels=m_ref)
        check(dx, want_dx, f"dL/dx ({tag})")
        if fold:
            _, dp2 = _lotd.lod_bwd(m, gt, xt, pt, None, need_input_grad=False, need_param_grad=True)
            check(dp2, want, f"dL/dparam without dL/dx ({tag})", levels=m_ref)
    for k in ("pair_fold", "pair_fixed", "pair_quad", "pair_direct"):
        hip_option(k, -1)
    if case != "c2":
        hip_option("lotd_pair", 0)
        check(_lotd.lod_bwd(m, gt, xt, pt, j, need_input_grad=True, need_param_grad=True)[1], want,
              "dL/dparam (lotd_pair = 0: corner records)", levels=m_ref)


@pytest.mark.parametrize("case", ["ngp_pair", "pair_f4"])
@pytest.mark.parametrize("kind", ["nan1", "inf1"])
def test_pair_path_dparam_half(oracle, inputs, dev, hip_option, case, kind):
    """half dL/dy and half tables: the kernels read half gradients and write a half dL/dparam themselves"""
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case)
    n = x.shape[0]
    gp = poison(g, kind, m.n_encoded_dims, n)
    g16, p16 = gp.astype(np.float16), p.astype(np.float16)
    want = oracle.lotd_bwd_dparam(m_ref, g16.astype(np.float32), x, p16.astype(np.float32), accum_double=True)
    xt, pt, gt = _t(dev, x, p16, g16)
    _, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
    for fold, fixed, quad, direct in PAIR_ROUTES:
        for k, val in (("pair_fold", fold), ("pair_fixed", fixed), ("pair_quad", quad), ("pair_direct", direct)):
            hip_option(k, val)
        dp = _lotd.lod_bwd(m, gt, xt, pt, j, need_input_grad=True, need_param_grad=True)[1]
        assert dp.dtype == torch.float16
        check(dp, want, f"half dL/dparam (fold={fold} fixed={fixed} quad={quad} direct={direct})", levels=m_ref, rel=HALF_TOL)


@pytest.mark.parametrize("case", ["hash_npow2", "dense_f8"])
@pytest.mark.parametrize("binned", [True, False])
@pytest.mark.parametrize("kind", ["nan1", "inf1"])
def test_generic_dparam(oracle, inputs, dev, monkeypatch, case, binned, kind):
    """generic corner records and the global-atomic path (USE_BINNED_DPARAM = False), first and second order"""
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case)
    monkeypatch.setattr(_lotd, "USE_BINNED_DPARAM", binned)
    n = x.shape[0]
    gp = poison(g, kind, m.n_encoded_dims, n)
    xt, pt, gt, vt = _t(dev, x, p, gp, v)
    check(_lotd.lod_bwd(m, gt, xt, pt, None, need_input_grad=False, need_param_grad=True)[1],
          oracle.lotd_bwd_dparam(m_ref, gp, x, p, accum_double=True), "dL/dparam", levels=m_ref)
    check(_lotd.lod_bwd_bwd_input(m, vt, gt, xt, pt, None, need_dLdinput_ddLdoutput=False, need_dLdinput_dparams=True,
                                  need_dLdinput_dinput=False)[1],
          oracle.lotd_bwd_bwd_dparam(m_ref, v, gp, x, p, accum_double=True), "d(dL/dx)/dparam", levels=m_ref)


# (cp_direct, vm_direct, direct_fixed, vm_sorted)
DIRECT_ROUTES = [(1, 1, 0, 0), (1, 1, 1, 0), (0, 0, 1, 0), (0, 0, 0, 0), (1, 1, 1, 2), (1, 1, 0, 2)]


@pytest.mark.parametrize("case", ["mixed", "mixed_smooth"])
@pytest.mark.parametrize("kind", ["nan1", "inf1", "table", "vin"])
def test_cp_vm_direct_dparam(oracle, inputs, dev, hip_option, case, kind):
    """k_cp_direct / k_vm_direct (s_bound: the workgroup's own bound) in fp64 and fixed point, and k_vm_sorted (gmax x the band's
    max |table value|): NaN / inf in dL/dy, NaN in table entries of the product levels (their updates multiply table values),
    NaN in dL/d(dL/dx) (second order)"""
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case)
    n = x.shape[0]
    gp, pp, vp = g, p, v
    if kind in ("nan1", "inf1"):
        gp = poison(g, kind, m.n_encoded_dims, n)
    elif kind == "table":
        pp = p.copy()
        for lvl, t in enumerate(LOTD_CASES[case][3]):
            if t in ("VM", "CP"):
                lo, hi = m.level_offsets[lvl], m.level_offsets[lvl + 1]
                pp[lo + (hi - lo) // 3] = np.nan
    else:
        vp = v.copy()
        vp[_rows(n)[1], 0] = np.nan
    xt, pt, gt, vt = _t(dev, x, pp, gp, vp)
    want1 = oracle.lotd_bwd_dparam(m_ref, gp, x, pp, accum_double=True) if kind != "vin" else None
    want2 = oracle.lotd_bwd_bwd_dparam(m_ref, vp, gp, x, pp, accum_double=True)
    for cp, vm, fixed, srt in DIRECT_ROUTES:
        for k, val in (("cp_direct", cp), ("vm_direct", vm), ("direct_fixed", fixed), ("vm_sorted", srt)):
            hip_option(k, val)
        tag = f"cp_direct={cp} vm_direct={vm} direct_fixed={fixed} vm_sorted={srt}"
        if want1 is not None:
            check(_lotd.lod_bwd(m, gt, xt, pt, None, need_input_grad=False, need_param_grad=True)[1], want1,
                  f"dL/dparam ({tag})", levels=m_ref)
        check(_lotd.lod_bwd_bwd_input(m, vt, gt, xt, pt, None, need_dLdinput_ddLdoutput=False, need_dLdinput_dparams=True,
                                      need_dLdinput_dinput=False)[1], want2, f"d(dL/dx)/dparam ({tag})", levels=m_ref)


@pytest.mark.parametrize("case", ["ngp_small", "mixed"])
def test_multi_pass_chunking(oracle, inputs, dev, hiplib, case):
    """2^10-point passes (as test_dparam_multi_pass_chunking): every pass takes a scale of its own"""
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case, n=5003, seed=12)
    gp = poison(g, "nan1", m.n_encoded_dims, x.shape[0])
    xt, pt, gt, vt = _t(dev, x, p, gp, v)
    want1 = oracle.lotd_bwd_dparam(m_ref, gp, x, p, accum_double=True)
    want2 = oracle.lotd_bwd_bwd_dparam(m_ref, v, gp, x, p, accum_double=True)
    hiplib.nr3d_lotd_set_dparam_chunk_log2(10)
    try:
        _, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
        dp = _lotd.lod_bwd(m, gt, xt, pt, j, need_input_grad=True, need_param_grad=True)[1]
        dp_b = _lotd.lod_bwd(m, gt, xt, pt, None, need_input_grad=False, need_param_grad=True)[1]
        dp2 = _lotd.lod_bwd_bwd_input(m, vt, gt, xt, pt, None, need_dLdinput_ddLdoutput=False, need_dLdinput_dparams=True,
                                      need_dLdinput_dinput=False)[1]
    finally:
        hiplib.nr3d_lotd_set_dparam_chunk_log2(0)
    check(dp, want1, "dL/dparam (chunked, fused)", levels=m_ref)
    check(dp_b, want1, "dL/dparam (chunked)", levels=m_ref)
    check(dp2, want2, "d(dL/dx)/dparam (chunked)", levels=m_ref)


@pytest.mark.parametrize("kind", ["nan1", "inf1", "vin"])
def test_forest_vm_sorted(oracle, dev, hip_option, kind):
    """a forest's VM levels over sorted points (k_vm_sorted; VsFix: the pass's max |dL/dy| x the band's max |table value|) in
    fixed point (direct_fixed = 1) and fp64 (0), and the record path (vm_sorted = 0), first and second order"""
    from nr3d_lib_amd import _hip
    from test_forest_gpu import _setup
    _lotd, fo, m_ref, metas, (x, p, g, v, bi), (xt, pt, _, _, bit) = _setup(oracle, dev, "plus", "vm_cuboid", n=20000, seed=31)
    n = x.shape[0]
    gp, vp = g, v
    if kind == "vin":
        vp = v.copy()
        vp[_rows(n)[1], 0] = np.nan
    else:
        gp = poison(g, kind, m_ref.as_dict()["n_encoded_dims"], n)
    gt, vt = _t(dev, gp, vp)
    want1 = oracle.lotd_forest_bwd_dparam(m_ref, fo, gp, x, p, block_inds=bi, accum_double=True)
    want2 = oracle.lotd_forest_bwd_dparam(m_ref, fo, gp, x, p, block_inds=bi, dL_ddLdx=vp, accum_double=True)
    _, j = _lotd.lod_fwd(metas, xt, pt, bit, need_input_grad=True)
    for srt, fixed in ((2, 1), (2, 0), (0, 1)):
        hip_option("vm_sorted", srt)
        hip_option("direct_fixed", fixed)
        _hip.prof_enable("lotd_direct")
        try:
            dp = _lotd.lod_bwd(metas, gt, xt, pt, None, bit, need_input_grad=False, need_param_grad=True)[1]
            dp2 = _lotd.lod_bwd_bwd_input(metas, vt, gt, xt, pt, j, bit, need_dLdinput_ddLdoutput=False, need_dLdinput_dparams=True,
                                          need_dLdinput_dinput=False)[1]
            ran = _hip.prof_read("lotd_direct")[1]
        finally:
            _hip.prof_enable()
        tag = f"vm_sorted={srt} direct_fixed={fixed}"
        assert (ran > 0) == (srt == 2), f"{tag}: the sorted kernel ran {ran} times"
        check(dp, want1, f"forest dL/dparam ({tag})", levels=m_ref, some_nonfinite=kind != "vin")
        check(dp2, want2, f"forest d(dL/dx)/dparam ({tag})", levels=m_ref)


# ---------------------------------------------------------------------------------------------------------------------
# LoTD second order on the pair path: d(dL/dx)/dparam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ngp_small", "ngp_pair", "pair_f4"])
@pytest.mark.parametrize("where", ["dy_one", "dy_both", "vin", "dy_inf"])
def test_pair_second_order_dparam(oracle, inputs, dev, hip_option, case, where):
    """k_pair_bin<SECOND>'s bound of an update is |g| x a bound on the weights: with NaN in only ONE feature of a pseudo level
    ('dy_one') a max that lets the NaN lose (fmaxf) kept the fixed point on and turned the NaN into a large finite number"""
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case)
    n = x.shape[0]
    gp, vp = g, v
    if where == "dy_one":
        gp = poison(g, "nan1", m.n_encoded_dims, n)
    elif where == "dy_both":
        gp = poison(g, "nan2", m.n_encoded_dims, n)
    elif where == "dy_inf":
        gp = poison(g, "inf1", m.n_encoded_dims, n)
    else:
        vp = v.copy()
        vp[_rows(n)[0], 1] = np.nan
        vp[_rows(n)[2], :] = np.inf
    xt, pt, gt, vt = _t(dev, x, p, gp, vp)
    want = oracle.lotd_bwd_bwd_dparam(m_ref, vp, gp, x, p, accum_double=True)
    for second, fixed, direct in itertools.product((1, 0), repeat=3):
        hip_option("pair_second", second)
        hip_option("pair_fixed", fixed)
        hip_option("pair_direct", direct)
        got = _lotd.lod_bwd_bwd_input(m, vt, gt, xt, pt, None, need_dLdinput_ddLdoutput=False, need_dLdinput_dparams=True,
                                      need_dLdinput_dinput=False)[1]
        check(got, want, f"d(dL/dx)/dparam (pair_second={second} pair_fixed={fixed} pair_direct={direct})", levels=m_ref)


# ---------------------------------------------------------------------------------------------------------------------
# LoTD dL/dx, dL/d(dL/dy) and d(dL/dx)/dx: a non-finite row makes exactly that row non-finite
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ngp_small", "hash_npow2", "mixed"])
@pytest.mark.parametrize("where", ["dy", "vin"])
def test_dx_and_hessian_rows(oracle, inputs, dev, hip_option, case, where):
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case)
    n = x.shape[0]
    gp, vp = g, v
    if where == "dy":
        gp = poison(g, "nan1", m.n_encoded_dims, n)
    else:
        vp = v.copy()
        vp[_rows(n)[1], 2] = np.nan
        vp[_rows(n)[2], 0] = -np.inf
    xt, pt, gt, vt = _t(dev, x, p, gp, vp)
    _, j_ref = oracle.lotd_fwd(m_ref, x, p, need_dydx=True)
    want_dx = oracle.lotd_bwd_dx(m_ref, gp, j_ref)
    want_ddy = oracle.lotd_bwd_bwd_ddLdy(m_ref, vp, j_ref)
    want_hx = oracle.lotd_bwd_bwd_dx(m_ref, vp, gp, x, p)
    _, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
    dx = _lotd.lod_bwd(m, gt, xt, pt, j, need_input_grad=True, need_param_grad=False)[0]
    check(dx, want_dx, "dL/dx", some_nonfinite=where == "dy")
    for levels_, pairlane, split in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        hip_option("hvp_levels", levels_)
        hip_option("hvp_pairlane", pairlane)
        hip_option("hvp_split", split)
        ddy, _, hx = _lotd.lod_bwd_bwd_input(m, vt, gt, xt, pt, j, need_dLdinput_ddLdoutput=True, need_dLdinput_dparams=False,
                                             need_dLdinput_dinput=True)
        tag = f"hvp_levels={levels_} hvp_pairlane={pairlane} hvp_split={split}"
        check(ddy, want_ddy, f"dL/d(dL/dy) ({tag})", some_nonfinite=where == "vin")
        check(hx, want_hx, f"d(dL/dx)/dx ({tag})")


# ---------------------------------------------------------------------------------------------------------------------
# LoTD forward: one NaN table entry per level
# ---------------------------------------------------------------------------------------------------------------------
def _nan_per_level(m, p):
    pp = p.copy()
    for lvl in range(m.n_levels):
        lo, hi = m.level_offsets[lvl], m.level_offsets[lvl + 1]
        pp[lo + (hi - lo) // 2] = np.nan
    return pp


@pytest.mark.parametrize("case", ["ngp_small", "hash_npow2", "mixed"])
def test_forward_nan_table_entry(oracle, inputs, dev, hip_option, case):
    """exactly the points that interpolate the NaN entry come out non-finite (y and dy/dx): two-lane forward against the
    corner sum (fwd_pairlane), one launch per level type against one launch (fwd_split); at 60 k points no level is staged
    in LDS (test_forward_nan_table_entry_lds_staged)"""
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case)
    pp = _nan_per_level(m, p)
    y_ref, j_ref = oracle.lotd_fwd(m_ref, x, pp, need_dydx=True)
    assert not np.isfinite(y_ref).all()
    xt, pt = _t(dev, x, pp)
    for pairlane, split in ((1, 1), (0, 1), (1, 0), (0, 0)):
        hip_option("fwd_pairlane", pairlane)
        hip_option("fwd_split", split)
        y, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
        tag = f"fwd_pairlane={pairlane} fwd_split={split}"
        check(y, y_ref, f"y ({tag})")
        check(j.reshape(j_ref.shape), j_ref, f"dy/dx ({tag})")


def _lds_levels(m, n):
    import ctypes
    from nr3d_lib_amd import _hip as H
    return H.lib().nr3d_lotd_fwd_lds_levels(ctypes.byref(m._cmeta()), n)


def test_forward_nan_table_entry_lds_staged(oracle, inputs, dev, hip_option):
    """the LDS-staged forward (fwd_lds_stage 1: coarse Dense tables whole in LDS) engages from 2^18 points on: at 2^19 + 77
    points the staged levels read their NaN entry from LDS, checked to be the case"""
    n = (1 << 19) + 77
    _lotd, m_ref, m, (x, p, g, v), _ = inputs("lds_stage", n=n)
    pp = _nan_per_level(m, p)
    xt, pt = _t(dev, x, pp)
    masks = {}
    for lds in (0, 1):
        hip_option("fwd_lds_stage", lds)
        masks[lds] = _lds_levels(m, n)
    assert masks[0] == 0
    assert masks[1] == 0b000011, bin(masks[1])                        # levels 0-1 whole
    outs = {}
    for lds in (0, 1):
        hip_option("fwd_lds_stage", lds)
        outs[lds] = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
    chunk = 1 << 17
    for s in range(0, n, chunk):                                      # the oracle's Jacobian in pieces (2^19 x 16 x 3)
        y_ref, j_ref = oracle.lotd_fwd(m_ref, x[s:s + chunk], pp, need_dydx=True)
        for lds, (y, j) in outs.items():
            check(y[s:s + chunk], y_ref, f"y (fwd_lds_stage={lds}, points {s}..)", some_nonfinite=False)
            check(j[s:s + chunk].reshape(j_ref.shape), j_ref, f"dy/dx (fwd_lds_stage={lds}, points {s}..)", some_nonfinite=False)
    for lds, (y, _) in outs.items():
        for lvl in range(5):                                          # every staged level reached its NaN entry
            assert not torch.isfinite(y[:, 2 * lvl:2 * lvl + 2]).all(), f"fwd_lds_stage={lds}: level {lvl} has no NaN"


# ---------------------------------------------------------------------------------------------------------------------
# folded route: non-finite values outside the served columns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("val", [np.nan, np.inf])
def test_nonfinite_outside_the_served_columns(oracle, inputs, dev, hip_option, val):
    """with max_level = 4 the columns of levels 5.. are not served: a NaN / inf there must not switch the pair path to fp64;
    the result is bit-identical to the same call with zeros there (extends test_largest_gradient_outside_the_served_columns)"""
    _lotd, m_ref, m, (x, p, g, v), _ = inputs("c2", n=200003, seed=5)
    hip_option("pair_fold", 1)
    gz = g.copy()
    gz[:, 2 * 5:] = 0.0
    gn = gz.copy()
    gn[99, -1] = val
    gn[100, 2 * 5] = val
    gn[101, 2 * 7 + 1] = -val
    xt, pt, gzt, gnt = _t(dev, x, p, gz, gn)
    _, j = _lotd.lod_fwd(m, xt, pt, max_level=4, need_input_grad=True)
    dx0, dp0 = _lotd.lod_bwd(m, gzt, xt, pt, j, max_level=4, need_input_grad=True, need_param_grad=True)
    dx1, dp1 = _lotd.lod_bwd(m, gnt, xt, pt, j, max_level=4, need_input_grad=True, need_param_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(dp0, dp1), "a non-finite value outside the served columns changed dL/dparam"
    # dL/dx sums every column (the reference's dL_dy . dy_dx, dy_dx zero outside the served levels): the rows with the
    # non-finite value are non-finite as the oracle's, every other row is unchanged
    keep = torch.ones(dx0.shape[0], dtype=torch.bool, device=dev)
    keep[99:102] = False
    assert torch.equal(dx0[keep], dx1[keep])
    _, j_ref = oracle.lotd_fwd(m_ref, x[99:102], p, max_level=4, need_dydx=True)
    check(dx1[99:102], oracle.lotd_bwd_dx(m_ref, gn[99:102], j_ref), "dL/dx of the rows with the non-finite value",
          some_nonfinite=False)
    assert_close(dp0, oracle.lotd_bwd_dparam(m_ref, gz, x, p, max_level=4, accum_double=True), name="dL/dparam", levels=m_ref)


# ---------------------------------------------------------------------------------------------------------------------
# magnitude edges of the fixed-point scales
# ---------------------------------------------------------------------------------------------------------------------
def _c2_calls(_lotd, m, xt, pt, gt, vt, hip_option):
    """(dL/dx, dL/dparam) on both pair_fold routes and d(dL/dx)/dparam, C2 at 2^20 points"""
    out = {}
    _, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
    for fold in (1, 0):
        hip_option("pair_fold", fold)
        out[f"fold{fold}"] = _lotd.lod_bwd(m, gt, xt, pt, j, need_input_grad=True, need_param_grad=True)
    hip_option("pair_fold", -1)
    out["second"] = (_lotd.lod_bwd_bwd_input(m, vt, gt, xt, pt, None, need_dLdinput_ddLdoutput=False, need_dLdinput_dparams=True,
                                             need_dLdinput_dinput=False)[1],)
    return out


@pytest.mark.parametrize("k", [-60, -20, 20, 60])
def test_power_of_two_equivariance(oracle, inputs, dev, hip_option, k):
    """the scale is 2^(lim - e): dL/dparam(2^k dy) = 2^k dL/dparam(dy) bit for bit, unless a clamp or a subnormal intervenes"""
    _lotd, m_ref, m, (x, p, g, v), cache = inputs("c2")
    xt, pt, gt, vt = _t(dev, x, p, g, v)
    if "base" not in cache:
        cache["base"] = _c2_calls(_lotd, m, xt, pt, gt, vt, hip_option)
    scaled = _c2_calls(_lotd, m, xt, pt, gt * 2.0 ** k, vt, hip_option)
    for route, outs in cache["base"].items():
        for nm, a, b in zip(("dL/dx", "dL/dparam") if len(outs) == 2 else ("d(dL/dx)/dparam",), outs, scaled[route]):
            want = a * 2.0 ** k
            assert torch.isfinite(want).all()
            assert torch.equal(b, want), f"{route} {nm}: {int((b != want).sum())} entries differ from 2^{k} x the unscaled call"


@pytest.mark.parametrize("k", [-100, 100])
def test_extreme_magnitudes_against_the_oracle(oracle, inputs, dev, hip_option, k):
    _lotd, m_ref, m, (x, p, g, v), cache = inputs("c2")
    gs = (g.astype(np.float64) * 2.0 ** k).astype(np.float32)
    xt, pt, gt = _t(dev, x, p, gs)
    want = oracle.lotd_bwd_dparam(m_ref, gs, x, p, accum_double=True)
    _, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
    for fold in (1, 0):
        hip_option("pair_fold", fold)
        dp = _lotd.lod_bwd(m, gt, xt, pt, j, need_input_grad=True, need_param_grad=True)[1]
        check(dp, want, f"dL/dparam x 2^{k} (fold={fold})", levels=m_ref, some_nonfinite=False)
    hip_option("pair_fold", -1)
    vt, = _t(dev, v)
    dp2 = _lotd.lod_bwd_bwd_input(m, vt, gt, xt, pt, None, need_dLdinput_ddLdoutput=False, need_dLdinput_dparams=True,
                                  need_dLdinput_dinput=False)[1]
    check(dp2, oracle.lotd_bwd_bwd_dparam(m_ref, v, gs, x, p, accum_double=True), f"d(dL/dx)/dparam x 2^{k}", levels=m_ref,
          some_nonfinite=False)


def _update_counts(_lotd, m, xt):
    """updates per dL/dparam entry: a bincount of the corner indices (lod_get_grid_index, bit-exact to the oracle's)"""
    cnt = torch.zeros(m.n_params, dtype=torch.int64, device=xt.device)
    for s in range(0, xt.shape[0], 1 << 17):
        gi = _lotd.lod_get_grid_index(m, xt[s:s + (1 << 17)])
        cnt += torch.bincount(gi.reshape(-1), minlength=m.n_params)
    return cnt.cpu().numpy()


def test_dynamic_range_across_levels(oracle, inputs, dev, hip_option):
    """the dL/dy columns of level l scaled by 2^(-2l) (down to 2^-30 on C2): one call-wide fixed-point scale.  A level whose
    fixed-point resolution (pair_fix_bits: 2^(e - lim) per update, max|g| < 2^e, lim = min(62 - sum_log2, 44)) times its
    largest update count is within REL_TOL of its own magnitude must meet REL_TOL; below that, every entry must be within the
    documented resolution times its update count (plus the fp32 rounding of the updates and of the result)"""
    _lotd, m_ref, m, (x, p, g, v), cache = inputs("c2")
    n = x.shape[0]
    col_level = np.repeat(np.arange(m.n_levels), 2)
    gs = (g.astype(np.float64) * 2.0 ** (-2.0 * col_level)[None, :]).astype(np.float32)
    xt, pt, gt = _t(dev, x, p, gs)
    want = oracle.lotd_bwd_dparam(m_ref, gs, x, p, accum_double=True)
    cnt = _update_counts(_lotd, m, xt)
    gmax = float(np.abs(gs).max())
    e = int(np.frexp(np.float32(gmax))[1])                           # gmax < 2^e (pair_fix_bits: (bits >> 23) - 126)
    sum_log2 = 3 + int(np.ceil(np.log2(n)))
    unit = 2.0 ** (e - min(62 - sum_log2, 44))
    _, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
    offs = list(m.level_offsets)
    for fold in (1, 0):
        hip_option("pair_fold", fold)
        dp = _np64(_lotd.lod_bwd(m, gt, xt, pt, j, need_input_grad=True, need_param_grad=True)[1])
        assert np.isfinite(dp).all()
        strict = []
        for lvl in range(m.n_levels):
            a, b = offs[lvl], offs[lvl + 1]
            w, d, c = want[a:b], dp[a:b], cnt[a:b]
            scale = float(np.abs(w).max())
            gl = float(np.abs(gs[:, 2 * lvl:2 * lvl + 2]).max())
            err = np.abs(d - w)
            if unit * float(c.max()) <= 0.1 * REL_TOL * scale:
                strict.append(lvl)
                assert float(err.max()) <= REL_TOL * scale, f"fold={fold} level {lvl}: {err.max():.3e} > REL_TOL x {scale:.3e}"
            else:
                bound = c * (unit + 4.0 * gl * 2.0 ** -24) + np.abs(w) * 2.0 ** -23
                bad = np.nonzero(err > bound)[0]
                assert bad.size == 0, (f"fold={fold} level {lvl}: entry {a + int(bad[0])} err {err[bad[0]]:.3e} > resolution bound "
                                       f"{bound[bad[0]]:.3e} ({int(c[bad[0]])} updates)")
        print(f"fold={fold}: levels held to REL_TOL of their own magnitude: {strict} of {m.n_levels}")
        assert strict[:4] == [0, 1, 2, 3]


@pytest.mark.parametrize("case", ["ngp_pair", "pair_f4"])
def test_zero_and_subnormal_gradients(oracle, inputs, dev, hip_option, case):
    """all-zero dL/dy: exact zeros on every fixed-point route; all-subnormal dL/dy (below 2^-126): finite, within a few fp32
    subnormal steps per update of the oracle (the device forms g w in fp32, the oracle in fp64)"""
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case)
    gsub = (g.astype(np.float64) * 2.0 ** -136).astype(np.float32)
    assert (np.abs(gsub) < 2.0 ** -126).all() and (gsub != 0).any()
    xt, pt, gzt, gst = _t(dev, x, p, np.zeros_like(g), gsub)
    want = oracle.lotd_bwd_dparam(m_ref, gsub, x, p, accum_double=True)
    cnt = _update_counts(_lotd, m, xt)
    _, j = _lotd.lod_fwd(m, xt, pt, need_input_grad=True)
    for fold, fixed, quad in itertools.product((1, 0), repeat=3):
        hip_option("pair_fold", fold)
        hip_option("pair_fixed", fixed)
        hip_option("pair_quad", quad)
        tag = f"fold={fold} fixed={fixed} quad={quad}"
        dp0 = _lotd.lod_bwd(m, gzt, xt, pt, j, need_input_grad=True, need_param_grad=True)[1]
        assert int(torch.count_nonzero(dp0)) == 0, f"zero dL/dy ({tag}): non-zero dL/dparam"
        dps = _np64(_lotd.lod_bwd(m, gst, xt, pt, j, need_input_grad=True, need_param_grad=True)[1])
        assert np.isfinite(dps).all(), tag
        err, bound = np.abs(dps - want), 4.0 * (cnt + 1) * 2.0 ** -149
        bad = np.nonzero(err > bound)[0]
        assert bad.size == 0, f"subnormal dL/dy ({tag}): entry {int(bad[0])} err {err[bad[0]]:.3e} ({int(cnt[bad[0]])} updates)"
        assert (dps != 0).sum() >= 0.5 * (want != 0).sum()


@pytest.mark.parametrize("case", ["mixed", "mixed_smooth"])
def test_zero_gradients_direct_routes(oracle, inputs, dev, hip_option, case):
    _lotd, m_ref, m, (x, p, g, v), _ = inputs(case)
    xt, pt, gzt, vt = _t(dev, x, p, np.zeros_like(g), v)
    for cp, vm, fixed, srt in DIRECT_ROUTES:
        for k, val in (("cp_direct", cp), ("vm_direct", vm), ("direct_fixed", fixed), ("vm_sorted", srt)):
            hip_option(k, val)
        dp = _lotd.lod_bwd(m, gzt, xt, pt, None, need_input_grad=False, need_param_grad=True)[1]
        dp2 = _lotd.lod_bwd_bwd_input(m, vt, gzt, xt, pt, None, need_dLdinput_ddLdoutput=False, need_dLdinput_dparams=True,
                                      need_dLdinput_dinput=False)[1]
        assert int(torch.count_nonzero(dp)) == 0 and int(torch.count_nonzero(dp2)) == 0, (cp, vm, fixed, srt)
