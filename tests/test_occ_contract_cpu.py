"""CPU: the float64 judge of the contracted march (tests/occ_contract_ref.py) pinned by hand-evaluated probes and by the oracle, and
the preconditions of the scenes the GPU tests march (tests/occ_contract_inputs.py).  Run with -s to read the undecided shares."""
import numpy as np
import pytest

import occ_contract_inputs as I
import occ_contract_ref as R

F = np.float32
_TRACES = {}


def oracle_trace(oracle, name, ctype):
    """every probe of the scene: the oracle's march through an all-ones grid, and the judge's verdict on it (shared, read-only)"""
    if (name, ctype) not in _TRACES:
        sc = I.scene(name)
        tr = oracle.ray_marching(sc["o"], sc["d"], sc["near"], sc["far"], *I.march_args(sc, np.ones(sc["res"], bool), ctype, I.TRACE_STEPS))
        _TRACES[name, ctype] = (sc, tr, R.judge(sc["o"], sc["d"], sc["roi"], sc["res"], ctype, tr[1], tr[2], tr[3]))
    return _TRACES[name, ctype]


def test_tanh_probe_by_hand():
    """ROI [-0.5, 0.5]^3, 32^3, o = (0, 0, 0.125), d = (1, 0.5, -0.25), (t0, t1) = (0.25, 0.75): tm = 0.5 and p = (0.5, 0.25, 0), all
    exact.  u = p + 0.5, so the tanh argument u - 0.5 is p itself:
      x  tanh(0.5)  = 0.46211716  -> c = 0.73105858  -> q = 23.393875  -> cell 23
      y  tanh(0.25) = 0.24491866  -> c = 0.62245933  -> q = 19.918699  -> cell 19
      z  tanh(0)    = 0           -> c = 0.5         -> q = 16 exactly: ON the interior face 16 -- cell 16, and undecided (15 is allowed)
    flat = (23 * 32 + 19) * 32 + 16 = 24176."""
    j = R.judge(np.array([[0, 0, 0.125]], F), np.array([[1, 0.5, -0.25]], F), I.ROI_POW2, (32, 32, 32), R.TANH,
                np.array([0.25], F), np.array([0.75], F), np.array([0]))
    assert j["p"].dtype == F and j["p"].tolist() == [[0.5, 0.25, 0.0]]
    np.testing.assert_allclose(j["c"][0], [0.73105858, 0.62245933, 0.5], rtol=0, atol=5e-9)
    np.testing.assert_allclose(j["q"][0], [23.393875, 19.918699, 16.0], rtol=0, atol=5e-7)
    assert j["cell"].tolist() == [[23, 19, 16]] and j["flat"].tolist() == [24176]
    assert j["undecided"].tolist() == [[False, False, True]] and j["face"][0, 2] == 16 and j["outside"] is None
    for gidx, verdict in ((24176, (False, False)), (24175, (False, True)), (24177, (True, False)), (24176 - 32, (True, False))):
        bad, excused = R.check_cells(j, np.array([gidx]), (32, 32, 32))       # 16 or, across the face, 15; never 17, never another axis
        assert (bool(bad[0]), bool(excused[0])) == verdict, gidx


def test_sphere_probes_by_hand():
    """ROI [-0.5, 0.5]^3, (20, 24, 28), o = 0, d = (0.75, 0, -1).
      (t0, t1) = (1.5, 2.5): tm = 2, p = (1.5, 0, -2); u = p + 0.5 = (2, 0.5, -1.5); v = 2 u - 1 = (3, 0, -4), n = 5 > 1: s = 2 - 1 / 5 =
        1.8, v / n = (0.6, 0, -0.8), s v / n = (1.08, 0, -1.44); c = that / 4 + 0.5 = (0.77, 0.5, 0.14); q = (15.4, 12, 3.92): cells
        (15, 12, 3), y exactly on the interior face 12 (undecided); flat = (15 * 24 + 12) * 28 + 3 = 10419.
      (t0, t1) = (0, 0.25): tm = 0.125, p = (0.09375, 0, -0.125); v = 2 p = (0.1875, 0, -0.25), n = 0.3125 <= 1: untouched;
        c = v / 4 + 0.5 = (0.546875, 0.5, 0.4375); q = (10.9375, 12, 12.25): cells (10, 12, 12); flat = (10 * 24 + 12) * 28 + 12 = 7068."""
    res = (20, 24, 28)
    j = R.judge(np.zeros((1, 3), F), np.array([[0.75, 0, -1]], F), I.ROI_POW2, res, R.SPHERE, np.array([1.5, 0], F),
                np.array([2.5, 0.25], F), np.array([0, 0]))
    assert j["p"].tolist() == [[1.5, 0.0, -2.0], [0.09375, 0.0, -0.125]]
    np.testing.assert_allclose(j["c"], [[0.77, 0.5, 0.14], [0.546875, 0.5, 0.4375]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(j["q"], [[15.4, 12, 3.92], [10.9375, 12, 12.25]], rtol=0, atol=1e-13)
    assert j["cell"].tolist() == [[15, 12, 3], [10, 12, 12]] and j["flat"].tolist() == [10419, 7068]
    assert j["outside"].tolist() == [True, False]
    assert j["undecided"].tolist() == [[False, True, False], [False, True, False]]
    assert R.unflatten(j["flat"], np.array(res)).tolist() == j["cell"].tolist()


def test_faces_zero_and_res_are_decided_and_delta():
    """far outside, the contracted coordinate sits on face 0 or face res, where the clamp puts both sides into the same cell: decided"""
    assert R.DELTA_ULPS == 16 and R.delta((32, 20, 64)).tolist() == [32 * 2.0 ** -20, 20 * 2.0 ** -20, 64 * 2.0 ** -20]
    j = R.judge(np.array([[30, -30, 0.25]], F), np.array([[0, 0, 0]], F), I.ROI_POW2, (32, 32, 32), R.TANH, np.zeros(1, F), np.ones(1, F), [0])
    assert j["cell"][0, :2].tolist() == [31, 0] and j["face"][0, :2].tolist() == [32, 0] and not j["undecided"][0, :2].any()


def test_filter_trace_by_hand():
    """two rays with probes in cells (1, 0, 1, 1 | 0, 1) of a grid with cell 1 occupied: cap 2 keeps probes 0, 2 and 5"""
    pi = np.array([[0, 4], [4, 0], [4, 2]], np.int32)
    ts = np.arange(6, dtype=F)[:, None]
    tr = [pi, ts, ts + 1, np.array([0, 0, 0, 0, 2, 2], np.int32), np.array([1, 0, 1, 1, 0, 1], np.int32)]
    out = R.filter_trace(tr, np.array([False, True]), 2, 3)
    assert out[0].tolist() == [[0, 2], [2, 0], [2, 1]] and out[0].dtype == np.int32
    assert out[1][:, 0].tolist() == [0, 2, 5] and out[3].tolist() == [0, 0, 2] and out[4].tolist() == [1, 1, 1]
    assert R.filter_trace(tr, np.array([False, True]), 9, 3)[0][:, 1].tolist() == [3, 0, 1]
    assert R.filter_trace(tr, np.array([False, False]), 9, 3)[1].shape == (0, 1)


@pytest.mark.parametrize("ctype", I.CTYPES)
@pytest.mark.parametrize("name", list(I.SCENES))
def test_oracle_agrees_with_the_judge_and_preconditions(oracle, name, ctype):
    sc, tr, j = oracle_trace(oracle, name, ctype)
    n, S = sc["o"].shape[0], tr[1].shape[0]
    pi = tr[0]
    assert n == 397 and pi[:, 1].max() < I.TRACE_STEPS, "the trace's cap lies above the longest probe sequence"
    assert pi[5, 1] == 0 and pi[6, 1] == 0 and sc["far"][5] == sc["near"][5] and sc["near"][6] > sc["far"][6]
    assert sc["d"][3].tolist() == [0, 0, 1] and pi[3, 1] > 0
    longest = int(pi[:, 1].max())
    assert all(c % g != 0 and c < longest for c in (7, 40, 65) for g in (16, 32, 64)) and set(I.CAPS) >= {1, 7, 40, 64, 65}, \
        "caps inside a look-ahead group, for every group size"
    assert (pi[:, 1] % 64 != 0).sum() > n // 2, "the far limit ends most rays in mid-group"
    # every probe: the oracle's cell is the float64 cell, or on an undecided axis its neighbour across that face
    bad, excused = R.check_cells(j, tr[4], sc["res"])
    und = j["undecided"].any(1)
    und_rays = R.ray_has(und, tr[3], n)
    print(f"\n{name} type {ctype}: {S} probes, longest ray {longest}; undecided {int(und.sum())} probes ({und.mean():.2e}) on {int(und_rays.sum())} "
          f"of {n} rays; the oracle takes the far side of the face on {int(excused.sum())}")
    assert not bad.any(), f"{int(bad.sum())} of {S} probes: the oracle's cell is neither the float64 cell nor excused by a tie"
    assert not (excused & ~und).any()
    # preconditions of the GPU tests
    assert und.mean() <= 1e-3, f"{und.mean():.2e} of the probes are undecided"
    assert und_rays.mean() <= 0.10, f"{und_rays.mean():.3f} of the rays contain an undecided probe"
    grid = I.scene_grids(sc["res"])["random"]
    occ = grid.ravel()[tr[4]]
    cnt = np.bincount(tr[3][occ], minlength=n)
    mixed = ((cnt > 0) & (cnt < pi[:, 1])).mean()
    assert mixed >= 0.60, f"only {mixed:.2f} of the rays have some but not all probes occupied"
    assert 0.4 < grid.mean() < 0.6 and 0 < I.scene_grids(sc["res"])["shell"].mean() < 0.2


@pytest.mark.parametrize("ctype", I.CTYPES)
@pytest.mark.parametrize("name", list(I.SCENES))
def test_filter_identity_holds_for_the_oracle(oracle, name, ctype):
    """the oracle's own march through a grid with a cap == the first `cap` occupied probes of its own trace: pins filter_trace, the
    host side of the GPU tests' exact check"""
    sc, tr, _ = oracle_trace(oracle, name, ctype)
    n = sc["o"].shape[0]
    for kind, grid in I.scene_grids(sc["res"]).items():
        for cap in I.CAPS:
            want = oracle.ray_marching(sc["o"], sc["d"], sc["near"], sc["far"], *I.march_args(sc, grid, ctype, cap))
            got = R.filter_trace(tr, grid, cap, n)
            for g, w, nm in zip(got, want, ["packed_info", "t_starts", "t_ends", "ridx", "gidx"]):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{kind} cap {cap}: {nm}"
            if kind == "random" and cap <= (7 if name == "outside" else 65):      # outside: 120 probes, long runs in one saturated cell
                assert (want[0][:, 1] == cap).sum() > 20, "the cap cuts rays off"


def test_gamma_scene_reaches_both_clamps_along_one_ray(oracle):
    sc, tr, _ = oracle_trace(oracle, "gamma", 1)
    raw = tr[1][:, 0] * F(sc["gamma"])                       # calc_dt clamps t0 * dt_gamma to [step, max_step]
    lo, hi = R.ray_has(raw < F(sc["step"]), tr[3], 397), R.ray_has(raw > F(sc["max_step"]), tr[3], 397)
    between = R.ray_has((raw > F(sc["step"])) & (raw < F(sc["max_step"])), tr[3], 397)
    assert (lo & hi & between).sum() >= 10, "rays that step by the lower clamp, by t * dt_gamma and by the upper clamp"


def test_outside_scene_leaves_the_roi(oracle):
    """a good part of every ray has |u| of 2 to 5; tanh saturates into the first and the last cell; the sphere's n > 1 branch is taken,
    left and taken again along a ray"""
    sc, tr, j = oracle_trace(oracle, "outside", 1)
    n, pi = 397, tr[0]
    u = (j["p"].astype(np.float64) - sc["roi"][:3]) / (sc["roi"][3:] - sc["roi"][:3])
    far_out = (np.abs(u).max(1) >= 2) & (np.abs(u).max(1) <= 5)
    share = np.bincount(tr[3], weights=far_out.astype(np.float64), minlength=n)[pi[:, 1] > 0] / pi[pi[:, 1] > 0, 1]
    assert share.min() >= 0.15 and share.mean() >= 0.5, (share.min(), share.mean())
    x = u - 0.5
    assert ((x > 2.5) & (j["cell"] == 31)).sum() > 1000, "saturated into the last cell"
    assert ((x < -2.5) & (j["cell"] == 0)).sum() > 1000, "saturated into the first cell"
    # a correctly rounded float32 tanh gives a coordinate of exactly 1.0f there: index == res, which only the clamp keeps inside
    one = np.tanh(x).astype(F) * F(0.5) + F(0.5) == F(1)
    assert one.any(1).sum() >= 10 and (j["cell"][one] == 31).all() and not j["undecided"][one].any()
    _, tr2, j2 = oracle_trace(oracle, "outside", 2)
    out = j2["outside"]
    pattern = 0
    for b, c in tr2[0]:
        s = out[b:b + c]
        pattern += bool(c and s[0] and not s.all() and s[-1])
    assert pattern >= 5 and (~out).sum() >= 50, (pattern, (~out).sum())


def test_batched_cases(oracle):
    """the batched route's inputs: -1 entries among the per-ray indices, a ray count the run length divides, one power-of-two ROI"""
    cases = I.batch_cases()
    bi = cases["batch_inds"][1]["batch_inds"]
    assert set(np.unique(bi)) == {-1, 0, 1, 2} and bi.shape[0] == 397
    cut, kw = cases["batch_data_size"]
    assert cut["o"].shape[0] == 396 == 3 * kw["batch_data_size"]
    ext = I.BATCH_ROI[:, 3:] - I.BATCH_ROI[:, :3]
    is_pow2 = lambda v: np.log2(v) == np.round(np.log2(v))
    assert is_pow2(ext[0]).all() and not is_pow2(ext[1]).any() and not is_pow2(ext[2]).any() and is_pow2(np.array(I.BATCH_RES)).all()
    # the oracle's batched trace against the judge, per entry
    for name, (sc, kw) in cases.items():
        tr = oracle.ray_marching(sc["o"], sc["d"], sc["near"], sc["far"], I.BATCH_ROI, I.batch_grids("full"), 1, sc["step"], sc["max_step"],
                                 sc["gamma"], I.TRACE_STEPS, True, **kw)
        vol = int(np.prod(I.BATCH_RES))
        j = R.judge(sc["o"], sc["d"], I.BATCH_ROI[tr[4]], I.BATCH_RES, 1, tr[1], tr[2], tr[3])
        assert (tr[5] // vol == tr[4]).all()
        bad, _ = R.check_cells(j, tr[5] - tr[4] * vol, I.BATCH_RES)
        assert not bad.any() and tr[0][:, 1].max() < I.TRACE_STEPS, name
        if "batch_inds" in kw:
            assert (tr[0][bi < 0, 1] == 0).all() and (tr[0][bi >= 0, 1] > 0).sum() > 200
