"""Permutohedral encoder on the GPU, the whole dispatch table and the inputs random points never reach (tests/permuto_inputs.py):
every compiled (D, pseudo width, table dtype) with its four kernels, points on faces of the simplices (rank ties) and on the
rounding tie of the nearest lattice point, tables of 1, 2 and 509 rows, the options and batching modes on the D > 16 loop path,
the layouts of dL/dy in the double backward, and non-finite positions.  The yardstick is the float64 restatement
(tests/permuto_ref.py); tests/test_permuto_inputs_cpu.py proves that the inputs reach those places and that these comparisons
would notice a wrong tie-break."""
import pytest
import torch

import permuto_inputs as I
import permuto_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # unit roundoff of float32


def _meta(c):
    from nr3d_lib_amd.bindings import _permuto as B
    m = B.PermutoEncMeta(c["D"], c["size"], I.RES, I.WIDTHS[c["width"]])
    assert m.n_feat_per_pseudo_lvl == c["width"] and m.n_params == c["meta"]["n_params"]
    return m


def _run(dev, c, dtype, x=None, gy=None, **kw):
    """forward, dL/dx + dL/dparam and the double backward of one case on the device: the four kernels of (D, width, dtype)"""
    from nr3d_lib_amd.bindings import _permuto as B
    m = _meta(c)
    xd = (c["x"] if x is None else x).to(dev)
    pd = c["p"].to(dtype).to(dev)
    gyd = c["gy"].to(dtype).to(dev) if gy is None else gy
    shd = c["shifts"].to(dev) if c["shifts"] is not None else None
    kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    y = B.permuto_enc_fwd(m, xd, pd, shd, **kw)
    dx, dp = B.permuto_enc_bwd(m, gyd, xd, pd, shd, need_input_grad=True, need_param_grad=True, **kw)
    ggy, dp2 = B.permuto_enc_bwd_bwd_input(m, c["ggx"].to(dev), gyd, xd, pd, shd, need_dL_ddLdy=True, need_dL_dparams=True, **kw)
    assert y.dtype == dtype and dx.dtype == torch.float32 and dp.dtype == dtype and ggy.dtype == dtype and dp2.dtype == dtype
    assert y.shape == (I.N, m.n_encoded_dims) and dx.shape == (I.N, c["D"]) and ggy.shape == y.shape
    return {"y": y, "dL_dx": dx, "dL_dparam": dp, "dL_ddLdy": ggy, "dL_dparam2": dp2}


@pytest.mark.parametrize("D,width,dtype", I.TABLE_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_every_table_entry(dev, D, width, dtype):
    """all 27 dimensions x 2 widths x 2 dtypes x 4 kernels = 432, on a 509-row table (prime, rows collide): 150 random points with
    shifts and 150 in (-8, 8)"""
    c = I.case(D, width, "table")
    I.compare_all(_run(dev, c, dtype), I.reference(D, width, "table"), dtype, c["levels"], tag=f"D={D} w={width}")


@pytest.mark.parametrize("D", I.FACE_DIMS)
@pytest.mark.parametrize("width", [2, 4])
@pytest.mark.parametrize("dtype", I.DTYPES, ids=["float32", "float16"])
@pytest.mark.parametrize("family", ["face", "half"])
def test_faces(dev, family, dtype, width, D):
    """points on faces of the simplices (ties of the rank comparison, decided by the reference's strict `<`) and on the rounding
    tie of the nearest remainder-0 point: y and dL/dparam to the usual bounds, dL/dx and dL/d(dL_dy) row by row, no row excused"""
    c = I.case(D, width, family)
    I.compare_all(_run(dev, c, dtype), I.reference(D, width, family), dtype, c["levels"], tag=f"{family} D={D} w={width}")


def _entry_bound(c):
    """per table entry: (number of addends n, sum of |addends| A, sum of |dL/dy| G) of dL/dparam, from the restatement"""
    r, x, sh = c["meta"], c["x"], c["shifts"]
    sc = I.scales_of(r)
    cnt = torch.zeros(r["n_params"], dtype=torch.float64)
    G = torch.zeros(r["n_params"], dtype=torch.float64)
    col = 0
    for lvl, (nf, size, off) in enumerate(zip(r["level_n_feats"], r["level_sizes"], r["level_offsets"])):
        _, rem0, rank = R.simplex(x, sc[lvl], sh[lvl] if sh is not None else None)
        rows = R.rows(rem0, rank, size)                                            # [N, D + 1]
        idx = off + rows[:, :, None] * nf + torch.arange(nf)[None, None, :]        # [N, D + 1, nf]
        g = c["gy"][:, None, col:col + nf].abs().double().expand(idx.shape)
        cnt.index_add_(0, idx.reshape(-1), torch.ones(idx.numel(), dtype=torch.float64))
        G.index_add_(0, idx.reshape(-1), g.reshape(-1))
        col += nf
    p64 = c["p"].double().requires_grad_(True)
    A, = torch.autograd.grad(R.encode(r, x, p64, shifts=sh), p64, c["gy"].abs().double())
    return cnt, A, G


@pytest.mark.parametrize("size", [1, 2, 509])
@pytest.mark.parametrize("D", [3, 20])
def test_small_and_odd_tables(dev, D, size):
    """Tables of 1, 2 and 509 rows (`h % size` with no power of two; with 1 or 2 rows every addend of a level lands in one or two
    rows).  The column-scale yardstick says little when thousands of addends meet in one entry, so every entry of dL/dparam
    (float32 table) is held to a bound of its own, u = 2^-24:

    The entry is the float32 sum, in any order, of n addends fl(g_t * w_t), g_t = dL/dy of the point and feature, w_t the
    barycentric weight of the vertex; the restatement's entry is the exact sum of g_t * W_t, W_t the weight computed exactly from
    the same float32 elevated coordinates.
      * weights: d = fl(elev - rem0) and delta = fl(d / (D+1)) carry two roundings, |delta^ - delta| <= 2u |delta| <= 3u
        (|delta| <= 1/2 at the nearest remainder-0 point, <= 3/2 once the `sum` correction has moved it by D+1); w_k =
        fl(delta_a - delta_b) adds u |w_k| <= u, so |w_k - W_k| <= 7u; w_0 = fl(delta_a + fl(1 - delta_b)) has one more rounding
        of a value <= 5/2: <= 9.5u.  Rounded up to 10u, the half u covering every product of two errors above.
      * the product and the n - 1 additions an addend goes through: n roundings, a factor within gamma_n = n u / (1 - n u) of 1
        (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1), in whatever order the atomics land.
    So |entry - restatement| <= gamma_n * A + (1 + gamma_n) * 10u * G, with A = sum |g_t| W_t (the restatement's dL/dparam for
    |dL/dy|; W_t >= 0) and G = sum |g_t| over the addends of the entry, n, A and G all from the restatement.  An entry no vertex
    maps to must be exactly zero.  No constant is fitted; the largest error / bound is printed.  y is held to the usual bound
    (with one row every weight multiplies the same values: dL/dx, dL/d(dL_dy) and the second-order dL/dparam are zero up to
    rounding there and have no scale to be held to), everything else to the usual bounds at 509 rows."""
    from nr3d_lib_amd.bindings import _permuto as B
    c = I.case(D, 2, "table", size)
    want = I.reference(D, 2, "table", size)
    m = _meta(c)
    xd, pd, shd = c["x"].to(dev), c["p"].to(dev), c["shifts"].to(dev)
    y = B.permuto_enc_fwd(m, xd, pd, shd)
    I.compare("y", y, want["y"], torch.float32, tag=f"size={size}")
    _, dp = B.permuto_enc_bwd(m, c["gy"].to(dev), xd, pd, shd, need_input_grad=False, need_param_grad=True)
    n, A, G = _entry_bound(c)
    assert int(n.sum()) == I.N * (D + 1) * sum(c["meta"]["level_n_feats"])
    gamma = n * U / (1 - n * U)
    bound = gamma * A + (1 + gamma) * 10 * U * G
    err = (dp.double().cpu() - want["dL_dparam"]).abs()
    assert (dp.cpu()[n == 0] == 0).all()
    live = n > 0
    ratio = float((err[live] / bound[live]).max())
    print(f"D={D} size={size}: max addends per entry {int(n.max())}, largest error / bound {ratio:.4f}")
    assert ratio <= 1.0
    if size == 509:
        I.compare_all(_run(dev, c, torch.float32), want, torch.float32, c["levels"], tag=f"size={size}")


LOOP_D = 24          # the D > 16 code path: vertex loops stay loops, pick / put select


def test_max_level_and_max_pos_dims_on_the_loop_path(dev):
    from nr3d_lib_amd.bindings import _permuto as B
    c = I.case(LOOP_D, 2, "table")
    m = _meta(c)
    want = I.compute_reference(c["meta"], c["x"], c["p"], c["gy"], c["ggx"], c["shifts"], max_level=0)
    xd, pd, gyd, shd, ggxd = (c[k].to(dev) for k in ("x", "p", "gy", "shifts", "ggx"))
    nf0 = c["meta"]["level_n_feats"][0]
    y = B.permuto_enc_fwd(m, xd, pd, shd, max_level=0)
    assert (y[:, nf0:] == 0).all()
    I.compare("y", y, want["y"], torch.float32, tag="max_level=0")
    dx, dp = B.permuto_enc_bwd(m, gyd, xd, pd, shd, None, None, None, 0, 5, True, True)
    assert (dx[:, 5:] == 0).all()
    I.compare("dL_dx", dx[:, :5], want["dL_dx"][:, :5], torch.float32, tag="max_level=0 max_pos_dims=5")
    I.compare("dL_dparam", dp, want["dL_dparam"], torch.float32, c["levels"], tag="max_level=0")
    assert (dp[c["meta"]["level_offsets"][1]:] == 0).all()
    ggy, dp2 = B.permuto_enc_bwd_bwd_input(m, ggxd, gyd, xd, pd, shd, max_level=0, need_dL_ddLdy=True, need_dL_dparams=True)
    assert (ggy[:, nf0:] == 0).all() and (dp2[c["meta"]["level_offsets"][1]:] == 0).all()
    I.compare("dL_ddLdy", ggy, want["dL_ddLdy"], torch.float32, tag="max_level=0")
    I.compare("dL_dparam2", dp2, want["dL_dparam2"], torch.float32, c["levels"], tag="max_level=0")
    assert (B.permuto_enc_fwd(m, xd, pd, shd, max_level=-1) == 0).all()
    assert B.permuto_enc_bwd(m, gyd, xd, pd, shd, max_level=-1, need_input_grad=True, need_param_grad=True) == (None, None)
    assert B.permuto_enc_bwd_bwd_input(m, ggxd, gyd, xd, pd, shd, max_level=-1, need_dL_ddLdy=True,
                                       need_dL_dparams=True) == (None, None)


@pytest.mark.parametrize("mode", ["bidx", "offsets", "batched"])
def test_batching_on_the_loop_path(dev, mode):
    """the three batching modes of test_batching at D = 24, with skipped points (batch_inds < 0) wherever indices are given"""
    n_sets = 3
    c = dict(I.case(LOOP_D, 2, "table"))
    g = torch.Generator().manual_seed(24)
    n_params = c["meta"]["n_params"]
    c["p"] = torch.randn(n_sets * n_params, generator=g).half().float()
    kw = {}
    if mode == "bidx":
        kw["batch_inds"] = torch.randint(-1, n_sets, (I.N,), generator=g)
    elif mode == "offsets":
        kw["batch_inds"] = torch.randint(-1, 2, (I.N,), generator=g)
        kw["batch_offsets"] = torch.tensor([2 * n_params, 0])
    else:
        kw["batch_data_size"] = I.N // n_sets
    want = I.compute_reference(c["meta"], c["x"], c["p"], c["gy"], c["ggx"], c["shifts"], bidx=kw.get("batch_inds"),
                               boffs=kw.get("batch_offsets"), bds=kw.get("batch_data_size", 0))
    got = _run(dev, c, torch.float32, **kw)
    I.compare_all(got, want, torch.float32, c["levels"], tag=mode)
    if "batch_inds" in kw:
        skipped = (kw["batch_inds"] < 0).to(dev)
        assert skipped.any()
        for k in ("y", "dL_dx", "dL_ddLdy"):
            assert (got[k][skipped] == 0).all(), k


@pytest.mark.parametrize("D", [7, LOOP_D])
@pytest.mark.parametrize("dtype", I.DTYPES, ids=["float32", "float16"])
def test_double_backward_layouts_of_dL_dy(dev, D, dtype):
    """dL/dy row-major, feature-major and expanded with stride 0 (as `y.sum().backward()` makes it): dL/d(dL_dy) agrees bit for
    bit between the three (one route of the kernel against another, as the dL/dx check of test_fwd_bwd_against_restatement), and
    with the restatement to the usual bound"""
    from nr3d_lib_amd.bindings import _permuto as B
    c = dict(I.case(D, 2, "table"))
    c["gy"] = torch.ones_like(c["gy"])
    want = I.compute_reference(c["meta"], c["x"], c["p"], c["gy"], c["ggx"], c["shifts"])
    m = _meta(c)
    xd, pd, shd, ggxd = c["x"].to(dev), c["p"].to(dtype).to(dev), c["shifts"].to(dev), c["ggx"].to(dev)
    E = m.n_encoded_dims
    row = torch.ones(I.N, E, dtype=dtype, device=dev)
    fm = torch.ones(E, I.N, dtype=dtype, device=dev).t()
    ex = torch.ones((), dtype=dtype, device=dev).expand(I.N, E)
    assert row.stride() == (E, 1) and fm.stride() == (1, I.N) and ex.stride() == (0, 0)
    outs = []
    for gy in (row, fm, ex):
        ggy, dp2 = B.permuto_enc_bwd_bwd_input(m, ggxd, gy, xd, pd, shd, need_dL_ddLdy=True, need_dL_dparams=True)
        I.compare("dL_ddLdy", ggy, want["dL_ddLdy"], dtype, tag=f"D={D} strides {tuple(gy.stride())}")
        I.compare("dL_dparam2", dp2, want["dL_dparam2"], dtype, c["levels"], tag=f"D={D} strides {tuple(gy.stride())}")
        dx, dp = B.permuto_enc_bwd(m, gy, xd, pd, shd, need_input_grad=True, need_param_grad=True)
        I.compare("dL_dx", dx, want["dL_dx"], dtype, tag=f"D={D} strides {tuple(gy.stride())}")
        I.compare("dL_dparam", dp, want["dL_dparam"], dtype, c["levels"], tag=f"D={D} strides {tuple(gy.stride())}")
        outs.append((ggy, dx))
    for ggy, dx in outs[1:]:
        assert torch.equal(ggy, outs[0][0]) and torch.equal(dx, outs[0][1])


BAD_ROWS = [0, 7, 63, 64, 149, 150, 255, 256, 298, 299]       # both halves of the points, block and wave boundaries, first and last


def _poison(x):
    """NaN, +-inf and 1e30 in 10 rows, one coordinate or all"""
    nan, inf = float("nan"), float("inf")
    x = x.clone()
    x[0] = nan
    x[7, 1] = nan
    x[63, 0] = inf
    x[64] = -inf
    x[149, -1] = 1e30
    x[150] = -1e30
    x[255, 0], x[255, 1] = inf, -inf
    x[256] = 3e38
    x[298, 0] = -nan
    x[299, -1] = -1e30
    return x


@pytest.mark.parametrize("D", [3, 20])
def test_non_finite_rows_stay_in_their_rows(dev, D):
    """every table access of the kernels is `row(k, size) * nf + c` with `row = h % size` on an unsigned h, and the rank-indexed
    arrays are built with selects, never a run-time index: in bounds for any bit pattern of x.  So NaN, +-inf and 1e30 in 10 rows
    leave every other row of y, dL/dx and dL/d(dL_dy) bit for bit what it is when those rows hold finite points; and with those
    rows skipped (batch_inds = -1) both parameter gradients meet the restatement.  Nothing is asserted about dL/dparam while the
    non-finite rows are live."""
    c = I.case(D, 2, "table")
    xb = _poison(c["x"])
    bad = torch.zeros(I.N, dtype=torch.bool)
    bad[BAD_ROWS] = True
    assert torch.equal(~torch.isfinite(xb).all(1) | (xb.abs() >= 1e30).any(1), bad)
    clean = _run(dev, c, torch.float32)
    dirty = _run(dev, c, torch.float32, x=xb)
    keep = (~bad).to(dev)
    for k in ("y", "dL_dx", "dL_ddLdy"):
        assert torch.isfinite(clean[k]).all()
        assert torch.equal(dirty[k][keep], clean[k][keep]), k
    bidx = torch.where(bad, -1, 0)
    want = I.compute_reference(c["meta"], c["x"], c["p"], c["gy"], c["ggx"], c["shifts"], bidx=bidx)
    got = _run(dev, c, torch.float32, x=xb, batch_inds=bidx)
    for k in ("y", "dL_dx", "dL_ddLdy"):
        assert (got[k][bad.to(dev)] == 0).all(), k
    I.compare_all(got, want, torch.float32, c["levels"], tag="non-finite rows skipped")
