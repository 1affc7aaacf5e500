"""GPU: csrc/knn.hip (nr3d_knn_points / nr3d_knn_points_backward) through ``nr3d_lib_amd.maths`` against the numpy restatement
tests/knn_ref.py.  On lattice inputs (exact in float32, full of ties) dists and idx are compared with ``torch.equal``; float inputs are
judged against float64 within the rounding bounds of knn_ref.  One sweep per axis around a small default, so that every K bucket, both
kernels (k_knn and k_knn_any), a partial wave, a partial tile, a tile boundary, every workgroup size and the several-queries-per-lane
variants are each reached.  Outputs are poisoned before every launch (tests/conftest.py), so an unwritten element shows: NaN and the
0xAB pattern equal nothing the restatement produces.

After the sweeps, every COMPILED kernel: coverage() maps each k_knn<D, KB, NORM, R> (80 with R = 1, 64 wide) and each k_knn_any<DC>
(9) to the named cases that run it; a case that claims a variant asks the launcher's own plan (launch_plan) before it launches, and
tests/test_knn_cpu.py checks the table for completeness and against that plan without a GPU."""
import os

import numpy as np
import pytest
import torch

import knn_ref as R
from nr3d_lib_amd import maths
from nr3d_lib_amd.maths import pytorch3d_knn as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_knn.npz")


@pytest.fixture(scope="module")
def B(hiplib):
    from nr3d_lib_amd.bindings import _pytorch3d_knn
    return _pytorch3d_knn


@pytest.fixture(autouse=True)
def every_call_on_the_kernel(monkeypatch):
    """by default a (D, K) off the fast kernel takes the torch route below GENERIC_MIN_ROWS query rows; here everything runs on the kernels"""
    monkeypatch.setattr(M, "GENERIC_MIN_ROWS", 0)


def test_generic_kernel_is_gated_by_size(dev, B, monkeypatch):
    monkeypatch.undo()
    assert M.FUSED_KNN is True and M.GENERIC_MIN_ROWS > 0
    few, many = torch.zeros(1, 70, 3, device=dev), torch.zeros(2, M.GENERIC_MIN_ROWS // 2, 3, device=dev)
    assert M._fused(few, 8) and M._fused(few, 32) and not M._fused(few, 33) and M._fused(many, 33)
    assert not M._fused(torch.zeros(1, 70, 9, device=dev), 1) and M._fused(torch.zeros(1, M.GENERIC_MIN_ROWS, 9, device=dev), 1)
    assert M._fused(few) and not M._fused(few.cpu(), 1) and not M._fused(few.cpu())
    monkeypatch.setattr(M, "FUSED_KNN", False)
    assert not M._fused(few, 1) and not M._fused(many, 33) and not M._fused(few)
    # the gated call gives the kernel's result
    monkeypatch.undo()
    rng = np.random.default_rng(0)
    p1, p2 = R.lattice(rng, (1, 70, 3), kmax=4), R.lattice(rng, (1, 90, 3), kmax=4)
    res = maths.knn_points(_d(p1, dev), _d(p2, dev), K=33)
    idx, dists = R.knn_points(p1, p2, K=33)
    assert _same(res, idx, dists)


def _d(a, dev, grad=False):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


def _same(res, idx, dists):
    return torch.equal(res.idx.cpu(), torch.from_numpy(idx)) and torch.equal(res.dists.detach().cpu(), torch.from_numpy(dists))


def _lattice_case(dev, norm, D, K, P1, P2, N, lengths=(None, None), kmax=4, seed=0):
    rng = np.random.default_rng(1000 * D + 10 * K + P1 + P2 + N + seed)
    p1, p2 = R.lattice(rng, (N, P1, D), kmax=kmax), R.lattice(rng, (N, P2, D), kmax=kmax)
    res = maths.knn_points(_d(p1, dev), _d(p2, dev), _d(lengths[0], dev), _d(lengths[1], dev), norm=norm, K=K)
    idx, dists = R.knn_points(p1, p2, lengths[0], lengths[1], norm, K)
    assert _same(res, idx, dists), (norm, D, K, P1, P2, N)


# ---- which named case runs which compiled kernel (csrc/knn.hip: launch_norm / launch_d / launch_kb and the switch of nr3d_knn_points)

BUCKETS = (1, 4, 8, 16, 32)                                      # KB
KS = (1, 2, 4, 5, 8, 9, 16, 17, 32)                              # both ends of every bucket
WIDE_R = {1: 4, 4: 2, 8: 2, 16: 2}                               # Wide<KB>::R; every wide case asks launch_plan for it before it launches
NARROW = [(D, K, norm) for D in range(1, 9) for K in KS for norm in (1, 2)]
NARROW_ROWS = (1, 70)                                            # N, P1: one partial workgroup of 64
WIDE = [(D, K, norm) for D in range(1, 9) for K in (1, 4, 8, 16) for norm in (1, 2)]
WIDE_ROWS = (512, 1000)                                          # R = 4: one group, all four strips live; R = 2: two groups, the second partial
GENERIC = [(D, K, norm) for D in range(1, 9) for K in (33, 40) for norm in (1, 2)] \
    + [(D, K, norm) for D in (9, 16) for K in (4, 33) for norm in (1, 2)]
GENERIC_ROWS = (3, 70)


def bucket(K):
    return next(kb for kb in BUCKETS if K <= kb)


def coverage():
    """{instantiation: [(case id, N, P1, D, K), ...]} with instantiation ("k_knn", D, KB, NORM, R) or ("k_knn_any", DC); N, P1, D, K
    are what the case launches, so that the plan it claims can be asked for without a GPU"""
    table = {}
    for D, K, norm in NARROW:
        table.setdefault(("k_knn", D, bucket(K), norm, 1), []).append((f"test_every_narrow_instantiation[{D}-{K}-{norm}]", *NARROW_ROWS, D, K))
    for D, K, norm in WIDE:
        table.setdefault(("k_knn", D, bucket(K), norm, WIDE_R[bucket(K)]), []).append(
            (f"test_every_wide_instantiation[{D}-{K}-{norm}]", *WIDE_ROWS, D, K))
    for D, K, norm in GENERIC:
        table.setdefault(("k_knn_any", D if D <= 8 else 0), []).append((f"test_every_generic_instantiation[{D}-{K}-{norm}]", *GENERIC_ROWS, D, K))
    return table


def test_fast_path_and_tile_queries(B):
    for D in range(1, 9):
        assert B.TILE(D) >= 64 and B.TILE(D) % 64 == 0
        for K in (1, 2, 4, 5, 8, 9, 16):
            assert B.fast_path(D, K)
    assert B.TILE(9) == 0 and B.TILE(0) == 0 and not B.fast_path(9, 1) and not B.fast_path(3, 10 ** 6) and not B.fast_path(0, 1)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 8, 9])
def test_lattice_sweep_D(dev, B, norm, D):
    assert B.fast_path(D, 4) == (D <= 8)
    _lattice_case(dev, norm, D, 4, 70, B.TILE(3) + 1, 1)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("K", [1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 40])
def test_lattice_sweep_K(dev, B, norm, K):
    """every bucket from both ends; 33 and 40 are above the largest one (k_knn_any)"""
    assert B.fast_path(3, K) == (K <= 32)
    _lattice_case(dev, norm, 3, K, 70, B.TILE(3) + 1, 1)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("P1", [1, 63, 70, 257])
def test_lattice_sweep_P1(dev, B, norm, P1):
    _lattice_case(dev, norm, 3, 4, P1, B.TILE(3) + 1, 1)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("where", ["1", "3", "T-1", "T", "T+1", "2T+3"])
@pytest.mark.parametrize("D,K", [(3, 4), (9, 4)])
def test_lattice_sweep_P2(dev, B, norm, where, D, K):
    T = B.TILE(3)
    P2 = {"1": 1, "3": 3, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[where]
    _lattice_case(dev, norm, D, K, 70, P2, 1)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("N", [1, 3])
def test_lattice_sweep_N(dev, B, norm, N):
    _lattice_case(dev, norm, 3, 4, 70, B.TILE(3) + 1, N)
    _lattice_case(dev, norm, 5, 8, 70, 2 * B.TILE(5) + 3, N, kmax=64)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K", [(3, 4), (3, 1), (8, 16), (9, 4), (3, 33)])
def test_ragged_lengths(dev, B, norm, D, K):
    """zero rows, zero padding (lengths2 < K, a zero length), every poisoned element overwritten"""
    T = B.TILE(3)
    _lattice_case(dev, norm, D, K, 70, T + 1, 3, lengths=(np.array([0, 37, 70]), np.array([2, T + 1, 0])))
    _lattice_case(dev, norm, D, K, 70, T + 1, 3, lengths=(np.array([70, 1, 69]), np.array([T, 1, T - 1])), seed=1)


@pytest.mark.parametrize("K,N,P1", [(1, 512, 300), (4, 512, 300), (8, 512, 300), (16, 512, 300), (17, 512, 300), (4, 300, 200)])
def test_launch_variants_against_the_restatement(dev, B, K, N, P1):
    """many clouds: 512 x 300 rows launch the several-queries-per-lane kernels with full workgroups (K = 17: one query per lane, full
    workgroups), 300 x 200 the half-size workgroup; the sweeps above run on single waves"""
    assert B.launch_plan(N, P1, 3, K) == ((1, 128) if N == 300 else (1, 256) if K == 17 else (WIDE_R[K], 256))
    rng = np.random.default_rng(K)
    l1, l2 = rng.integers(0, P1 + 1, N), rng.integers(0, 8, N)
    l1[:2], l2[:2] = P1, 7
    _lattice_case(dev, 2, 3, K, P1, 7, N, lengths=(l1, l2))


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("K", [1, 4, 8, 16, 17])
def test_launch_variants_across_tiles_against_the_torch_route(dev, B, monkeypatch, norm, K):
    """the same launches over a tile boundary, against the pure-torch route on the same device (the restatement takes too long here;
    the route itself is compared with it in test_both_routes_agree and on the CPU)"""
    assert B.launch_plan(512, 300, 3, K) == ((1, 256) if K == 17 else (WIDE_R[K], 256))
    _across_tiles_against_the_torch_route(dev, B, monkeypatch, norm, 3, K)


def _across_tiles_against_the_torch_route(dev, B, monkeypatch, norm, D, K):
    N, P1, P2 = 512, 300, B.TILE(D) + 1
    rng = np.random.default_rng(K)
    p1, p2 = _d(R.lattice(rng, (N, P1, D), kmax=4), dev), _d(R.lattice(rng, (N, P2, D), kmax=4), dev)
    l1, l2 = rng.integers(0, P1 + 1, N), rng.integers(0, P2 + 1, N)
    l1[:2], l2[:2] = P1, P2
    got = maths.knn_points(p1, p2, _d(l1, dev), _d(l2, dev), norm=norm, K=K)
    monkeypatch.setattr(M, "FUSED_KNN", False)
    want = maths.knn_points(p1, p2, _d(l1, dev), _d(l2, dev), norm=norm, K=K)
    assert torch.equal(got.idx, want.idx) and torch.equal(got.dists, want.dists)


# ---- every compiled kernel (coverage() above names these cases)

@pytest.mark.parametrize("D,K,norm", NARROW)
def test_every_narrow_instantiation(dev, B, D, K, norm):
    """k_knn<D, KB, NORM, 1> for every D, both ends of every bucket, both norms: a partial wave (70 rows) over a tile boundary (T + 1
    candidates).  D = 5, 6, 7: the LDS row is 8 floats wide and read_row fetches padding that nothing has written, which must not
    reach a distance.  Once on the tie-heavy lattice (9 values per coordinate) and, at the top K of a bucket, once more on the spread
    one (lattice_kmax(D)), where insert() sorts mostly distinct distances."""
    assert B.launch_plan(*NARROW_ROWS, D, K) == (1, 64)
    _lattice_case(dev, norm, D, K, NARROW_ROWS[1], B.TILE(D) + 1, NARROW_ROWS[0])
    if K in BUCKETS:
        _lattice_case(dev, norm, D, K, NARROW_ROWS[1], B.TILE(D) + 1, NARROW_ROWS[0], kmax=None)


def _wide_case(dev, B, norm, D, K, N, P1, P2=7):
    """ragged clouds for a launch of Rw queries per lane in 256 lanes: clouds 0 and 1 full; cloud 2 empty; cloud 3 ends exactly where the
    second group of 256 Rw rows begins (a group of padding rows only, when there is one), cloud 4 one row later; cloud 5 fills the first
    strip only"""
    Rw = WIDE_R[bucket(K)]
    assert B.launch_plan(N, P1, D, K) == (Rw, 256)
    rng = np.random.default_rng(100 * D + K)
    l1, l2 = rng.integers(0, P1 + 1, N), rng.integers(0, P2 + 1, N)
    l1[:2], l2[:2] = P1, P2
    l1[2:6], l2[2:6] = [0, min(256 * Rw, P1 - 1), min(256 * Rw + 1, P1), 256], P2
    _lattice_case(dev, norm, D, K, P1, P2, N, lengths=(l1, l2))


@pytest.mark.parametrize("D,K,norm", WIDE)
def test_every_wide_instantiation(dev, B, D, K, norm):
    """k_knn<D, KB, NORM, R> with R = 4 (K = 1) and R = 2 (KB = 4, 8, 16): 1000 rows per cloud put live rows into all four strips of
    R = 4 and give R = 2 two groups per cloud (first = g wg R with g > 0), the second one partial; a cloud of at most 512 rows leaves
    that second group with padding rows only (the len2 = 0 shortcut: zeros written, nothing searched)"""
    _wide_case(dev, B, norm, D, K, *WIDE_ROWS)


@pytest.mark.parametrize("norm", [1, 2])
def test_wide_second_group_of_one_row(dev, B, norm):
    """R = 4 with two groups per cloud, the second holding the single row 1024"""
    _wide_case(dev, B, norm, 3, 1, 256, 1025)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K", [(8, 16), (6, 4), (1, 1)])
def test_wide_variants_across_tiles_with_other_D(dev, B, monkeypatch, norm, D, K):
    """the wide variants over a tile boundary at the widest, a padded and the narrowest LDS row, against the pure-torch route on the
    same device (on the lattice the two arithmetics agree bit for bit)"""
    assert B.launch_plan(512, 300, D, K) == (WIDE_R[bucket(K)], 256)
    _across_tiles_against_the_torch_route(dev, B, monkeypatch, norm, D, K)


@pytest.mark.parametrize("D,K,norm", GENERIC)
def test_every_generic_instantiation(dev, B, D, K, norm):
    """k_knn_any<DC>: DC = 1 .. 8 above the largest bucket, and the runtime-D loop (DC = 0) at D = 9 and 16; len2 % 4 = 2 (P2 = 2, 6)
    beside the 0, 1 and 3 of the P2 sweep; lengths2 below K, a zero length and a row limit in every call"""
    N, P1 = GENERIC_ROWS
    assert B.launch_plan(N, P1, D, K) is None and not B.fast_path(D, K)
    for P2 in (2, 6, B.TILE(3) + 1):
        _lattice_case(dev, norm, D, K, P1, P2, N, lengths=(np.array([P1, 37, P1 - 1]), np.array([P2, min(P2, 3), max(P2 - 2, 0)])))


# ---- insert(): directed orders

@pytest.mark.parametrize("D,K,norm", [(D, K, norm) for K in BUCKETS for D in (1, 3, 7) for norm in (1, 2)])
def test_insert_on_directed_orders(dev, B, D, K, norm):
    """each bucket at its top K on four clouds of T + 1 candidates that differ in coordinate 0 only (knn_ref.directed_p2), against
    queries with coordinate 0 <= 0: descending distance (every candidate enters at slot 0 and shifts the whole list, the first
    candidate of the second tile included), ascending (nothing enters once the list is full), far and near in turns, all equal (the
    first K indices, in order).  Every distance is one exact square or absolute value plus a constant of the row; three of the four
    answers are also written down in closed form, which pins the restatement."""
    orders = ("descending", "ascending", "alternating", "equal")
    P1, P2 = 70, B.TILE(D) + 1
    assert (P2 + 4) ** 2 + 16 * (D - 1) < 2 ** 24 and B.launch_plan(len(orders), P1, D, K) == (1, 64) and K <= P2
    rng = np.random.default_rng(10 * D + K)
    a = R.lattice(rng, (P1, D), kmax=4)
    a[:, 0] = -np.abs(a[:, 0])
    p1 = np.broadcast_to(a, (len(orders), P1, D)).copy()
    p2 = np.stack([R.directed_p2(D, o, P2) for o in orders])
    res = maths.knn_points(_d(p1, dev), _d(p2, dev), norm=norm, K=K)
    idx, dists = R.knn_points(p1, p2, norm=norm, K=K)
    assert _same(res, idx, dists)
    f = np.square if norm == 2 else np.abs
    a64, k = a.astype(np.float64), np.arange(K)
    rest = f(a64[:, 1:]).sum(1)[:, None]
    # the k-th neighbour: its index and the numerator of its coordinate 0
    for n, want_idx, k0 in ((0, P2 - 1 - k, k), (1, k, k), (3, k, np.full(K, 3))):
        assert np.array_equal(idx[n], np.broadcast_to(want_idx, (P1, K))), orders[n]
        assert np.array_equal(dists[n], (f(k0[None, :] / 256.0 - a64[:, :1]) + rest).astype(np.float32)), orders[n]


# ---- the two guards of the contract: lengths outside [0, P], idx outside [0, P2)

@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K,N,P1,plan", [(3, 4, 16, 70, (1, 64)), (3, 4, 512, 300, (2, 256)), (3, 33, 16, 70, None)])
def test_lengths_outside_the_cloud_are_clamped(dev, B, norm, D, K, N, P1, plan):
    """-5, -1, P + 1, 2^40, INT64_MIN and INT64_MAX in lengths1 and lengths2 (knn_ref.wild_lengths), through the binding, on a narrow,
    a wide and the generic kernel and on the backward: each is clamped into [0, P] (clamp_len guards every use of a length in
    csrc/knn.hip), so the result is the restatement's with np.clip"""
    P2 = 7
    assert B.launch_plan(N, P1, D, K) == plan
    rng = np.random.default_rng(N + K)
    p1, p2 = R.lattice(rng, (N, P1, D), kmax=8), R.lattice(rng, (N, P2, D), kmax=8)
    l1, l2 = R.wild_lengths(rng, N, P1), R.wild_lengths(rng, N, P2, at=8)
    gd = (2.0 ** rng.integers(-2, 3, size=(N, P1, K))).astype(np.float32)
    assert P1 * K * (2 * 4 * 16 / 256) * 2 ** 9 < 2 ** 24          # exact sums, as in test_backward_exact_on_the_lattice
    got_idx, got_d = B.knn_points_idx(_d(p1, dev), _d(p2, dev), _d(l1, dev), _d(l2, dev), norm, K)
    idx, dists = R.knn_points(p1, p2, l1, l2, norm, K)
    assert idx.any() and torch.equal(got_idx.cpu(), torch.from_numpy(idx)) and torch.equal(got_d.cpu(), torch.from_numpy(dists))
    g1, g2 = B.knn_points_backward(_d(p1, dev), _d(p2, dev), _d(l1, dev), _d(l2, dev), got_idx, norm, _d(gd, dev))
    w1, w2 = R.knn_backward(p1, p2, l1, l2, idx, norm, gd)[:2]
    assert w1.any() and torch.equal(g1.cpu().double(), torch.from_numpy(w1)) and torch.equal(g2.cpu().double(), torch.from_numpy(w2))


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K", [(3, 8), (9, 3)])
def test_backward_skips_idx_outside_the_cloud(dev, B, norm, D, K):
    """the idx of a real forward with a tenth of its entries overwritten by -1, P2, P2 + 7 and 2^40: those (n, i, k) terms are missing
    from BOTH gradients and nothing else changes (k_knn_bwd tests j before every access through it); exact sums, as above"""
    N, P1, P2 = 2, 300, 5
    rng = np.random.default_rng(D + K)
    p1, p2 = R.lattice(rng, (N, P1, D), kmax=8), R.lattice(rng, (N, P2, D), kmax=8)
    gd = (2.0 ** rng.integers(-2, 3, size=(N, P1, K))).astype(np.float32)
    for lens in ((None, None), (np.array([299, 120]), np.array([5, 2]))):
        idx = R.knn_points(p1, p2, lens[0], lens[1], norm, K)[0]
        bad, hit = R.spoil_idx(rng, idx, P2)
        assert all((bad == v).any() for v in (-1, P2, P2 + 7, 2 ** 40))
        g1, g2 = B.knn_points_backward(_d(p1, dev), _d(p2, dev), _d(lens[0], dev), _d(lens[1], dev), _d(bad, dev), norm, _d(gd, dev))
        w1, w2 = R.knn_backward(p1, p2, lens[0], lens[1], bad, norm, gd)[:2]
        clean = R.knn_backward(p1, p2, lens[0], lens[1], idx, norm, gd)[:2]
        assert not np.array_equal(w1, clean[0]) and not np.array_equal(w2, clean[1])
        assert torch.equal(g1.cpu().double(), torch.from_numpy(w1)) and torch.equal(g2.cpu().double(), torch.from_numpy(w2))


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_return_nn_and_gradients_equal_the_reference_wrapper(dev, B, tag):
    golden = np.load(GOLDEN)
    g = {k[2:]: golden[k] for k in golden.files if k.startswith(tag + "_")}
    p1, p2 = _d(g["p1"], dev, grad=True), _d(g["p2"], dev, grad=True)
    l1, l2 = _d(golden["lengths1"], dev), _d(golden["lengths2"], dev)
    res = maths.knn_points(p1, p2, l1, l2, norm=int(g["norm"]), K=int(g["K"]), return_nn=True)
    assert _same(res, g["idx"], g["dists"]) and torch.equal(res.knn.detach().cpu(), torch.from_numpy(g["knn"]))
    g1, g2 = torch.autograd.grad(res.dists, (p1, p2), _d(g["grad_dists"], dev))
    assert torch.equal(g1.cpu(), torch.from_numpy(g["grad_p1"])) and torch.equal(g2.cpu(), torch.from_numpy(g["grad_p2"]))
    again = maths.knn_points(p1, p2, l1, l2, norm=int(g["norm"]), K=int(g["K"]), version=2, return_sorted=False)
    assert torch.equal(again.idx, res.idx) and torch.equal(again.dists, res.dists)


def test_empty_clouds(dev, B):
    for s1, s2 in (((0, 4, 3), (0, 5, 3)), ((2, 0, 3), (2, 5, 3)), ((2, 4, 3), (2, 0, 3))):
        a, b = torch.zeros(s1, device=dev, requires_grad=True), torch.zeros(s2, device=dev, requires_grad=True)
        res = maths.knn_points(a, b, K=2, return_nn=True)
        assert res.dists.shape == (s1[0], s1[1], 2) and not res.dists.any() and not res.idx.any() and not res.knn.any()
        g1, g2 = torch.autograd.grad(res.dists.sum(), (a, b))
        assert g1.shape == a.shape and g2.shape == b.shape and not g1.any() and not g2.any()


def test_entry_refuses_bad_arguments(dev, B):
    from nr3d_lib_amd import _hip as H
    l = H.lib()
    x = torch.zeros(8, device=dev)
    i = torch.zeros(8, dtype=torch.int64, device=dev)
    for args, word in (((1, 1, 1, 3, 0, 2), "K = 0"), ((1, 1, 1, 0, 1, 2), "D = 0"), ((1, 1, 1, 3, 1, 3), "norm = 3"),
                       ((1, 2 ** 31, 1, 3, 1, 2), "2^31"), ((1, 1, 2 ** 31, 3, 1, 2), "2^31")):
        assert l.nr3d_knn_points(H.ptr(x), H.ptr(x), None, None, *args, H.ptr(x), H.ptr(i), H.stream_of(x)) != 0
        assert word in l.nr3d_last_error().decode()
        assert l.nr3d_knn_points_backward(H.ptr(x), H.ptr(x), None, None, H.ptr(i), H.ptr(x), *args, H.ptr(x), H.ptr(x), H.stream_of(x)) != 0
        assert word in l.nr3d_last_error().decode()
    torch.cuda.synchronize()
    assert not x.any() and not i.any()


# ---- float inputs

@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("K", [1, 8])
def test_float_inputs_within_the_rounding_bound(dev, B, norm, K):
    _float_case(dev, B, norm, 3, K)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K", [(1, 4), (5, 16), (8, 32), (6, 33)])
def test_float_inputs_within_the_rounding_bound_beyond_D3(dev, B, norm, D, K):
    """the narrowest row, a padded LDS row, the widest row with the longest list, and the generic kernel; the bound is knn_ref's"""
    assert B.fast_path(D, K) == (K <= 32)
    _float_case(dev, B, norm, D, K)


def _float_case(dev, B, norm, D, K):
    P1, P2 = 300, 2 * B.TILE(3) + 3
    rng = np.random.default_rng(K)
    p1, p2 = R.normal(rng, (1, P1, D)), R.normal(rng, (1, P2, D))
    res = maths.knn_points(_d(p1, dev), _d(p2, dev), norm=norm, K=K)
    d, idx = res.dists.cpu().numpy()[0].astype(np.float64), res.idx.cpu().numpy()[0]
    assert idx.min() >= 0 and idx.max() < P2 and all(len(set(r)) == K for r in idx.tolist())
    assert np.all(np.diff(d, axis=1) >= 0)
    d64 = R.pair_dists64(p1[0], p2[0], norm)
    assert np.all(np.abs(d - np.take_along_axis(d64, idx, 1)) <= R.dist_bound(D, d))
    rest = d64.copy()
    np.put_along_axis(rest, idx, np.inf, 1)
    assert np.all(rest.min(1) >= d[:, -1] - R.dist_bound(D, d[:, -1]))


def test_forward_is_deterministic(dev, B):
    rng = np.random.default_rng(5)
    p1, p2 = _d(R.normal(rng, (2, 300, 3)), dev), _d(R.lattice(rng, (2, 2 * B.TILE(3) + 3, 3), kmax=2), dev)
    a, b = maths.knn_points(p1, p2, K=8), maths.knn_points(p1, p2, K=8)
    assert torch.equal(a.dists.view(torch.int32), b.dists.view(torch.int32)) and torch.equal(a.idx, b.idx)


@pytest.mark.parametrize("K", [4, 33])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_rows_stay_in_their_rows(dev, B, K, bad):
    N, P1, P2 = 3, 200, B.TILE(3) + 7
    rng = np.random.default_rng(9)
    p1, p2 = R.normal(rng, (N, P1, 3)), R.normal(rng, (N, P2, 3))
    l2 = np.array([P2, P2 - 5, 3])
    clean = maths.knn_points(_d(p1, dev), _d(p2, dev), None, _d(l2, dev), K=K)
    limit = torch.from_numpy(np.maximum(l2, 1)).to(dev)[:, None, None]
    # 5 % of the p1 rows: every other row as in the clean run
    hit = rng.random((N, P1)) < 0.05
    q1 = p1.copy()
    q1[hit, rng.integers(0, 3, int(hit.sum()))] = bad
    res = maths.knn_points(_d(q1, dev), _d(p2, dev), None, _d(l2, dev), K=K)
    keep = torch.from_numpy(~hit).to(dev)
    assert torch.equal(res.idx[keep], clean.idx[keep]) and torch.equal(res.dists[keep], clean.dists[keep])
    assert bool(((res.idx >= 0) & (res.idx < limit)).all())
    # 5 % of the p2 rows of cloud 1: clouds 0 and 2 as in the clean run
    q2 = p2.copy()
    hit2 = rng.random(P2) < 0.05
    q2[1, hit2, 0] = bad
    res = maths.knn_points(_d(p1, dev), _d(q2, dev), None, _d(l2, dev), K=K)
    assert torch.equal(res.idx[[0, 2]], clean.idx[[0, 2]]) and torch.equal(res.dists[[0, 2]], clean.dists[[0, 2]])
    assert bool(((res.idx >= 0) & (res.idx < limit)).all())


# ---- backward

@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K", [(3, 2), (3, 8), (9, 3)])
def test_backward_exact_on_the_lattice(dev, B, norm, D, K):
    """power-of-two grad_dists on lattice points: every sum is exact (fewer than 2^24 quanta of 2^-9), so the atomics' order cannot
    show; P2 = 5 against P1 = 300 forces many hits on one p2 element"""
    N, P1, P2 = 2, 300, 5
    rng = np.random.default_rng(D + K)
    p1, p2 = R.lattice(rng, (N, P1, D), kmax=8), R.lattice(rng, (N, P2, D), kmax=8)
    gd = (2.0 ** rng.integers(-2, 3, size=(N, P1, K))).astype(np.float32)
    assert P1 * K * (2 * 4 * 16 / 256) * 2 ** 9 < 2 ** 24
    for lens in ((None, None), (np.array([299, 120]), np.array([5, 2]))):
        a, b = _d(p1, dev, grad=True), _d(p2, dev, grad=True)
        res = maths.knn_points(a, b, _d(lens[0], dev), _d(lens[1], dev), norm=norm, K=K)
        idx, dists = R.knn_points(p1, p2, lens[0], lens[1], norm, K)
        assert _same(res, idx, dists)
        g1, g2 = torch.autograd.grad(res.dists, (a, b), _d(gd, dev))
        w1, w2 = R.knn_backward(p1, p2, lens[0], lens[1], idx, norm, gd)[:2]
        assert torch.equal(g1.cpu().double(), torch.from_numpy(w1)) and torch.equal(g2.cpu().double(), torch.from_numpy(w2))


@pytest.mark.parametrize("norm", [1, 2])
def test_backward_float_inputs_within_the_rounding_bound(dev, B, norm):
    N, P1, P2, K = 2, 300, 50, 8
    rng = np.random.default_rng(3)
    p1, p2, gd = R.normal(rng, (N, P1, 3)), R.normal(rng, (N, P2, 3)), R.normal(rng, (N, P1, K))
    a, b = _d(p1, dev, grad=True), _d(p2, dev, grad=True)
    res = maths.knn_points(a, b, norm=norm, K=K)
    g1, g2 = torch.autograd.grad(res.dists, (a, b), _d(gd, dev))
    w1, w2, s1, s2, m2 = R.knn_backward(p1, p2, None, None, res.idx.cpu().numpy(), norm, gd)
    assert m2.max() > 8
    assert np.all(np.abs(g1.cpu().numpy() - w1) <= (K + 3) * R.EPS * s1)
    assert np.all(np.abs(g2.cpu().numpy() - w2) <= (m2[..., None] + 3) * R.EPS * s2)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K", [(3, 4), (9, 33)])
def test_both_routes_agree(dev, B, monkeypatch, norm, D, K):
    """FUSED_KNN False (pure torch on the GPU) equals True (the kernel) on the lattice, forward and backward, and the restatement"""
    N, P1, P2 = 3, 70, B.TILE(3) + 1
    rng = np.random.default_rng(D)
    p1, p2 = R.lattice(rng, (N, P1, D), kmax=8), R.lattice(rng, (N, P2, D), kmax=8)
    l1, l2 = np.array([0, 37, 70]), np.array([2, P2, 0])
    gd = (2.0 ** rng.integers(-2, 3, size=(N, P1, K))).astype(np.float32)
    out = []
    for fused in (True, False):
        monkeypatch.setattr(M, "FUSED_KNN", fused)
        a, b = _d(p1, dev, grad=True), _d(p2, dev, grad=True)
        res = maths.knn_points(a, b, _d(l1, dev), _d(l2, dev), norm=norm, K=K, return_nn=True)
        out.append((res.dists.detach(), res.idx, res.knn.detach()) + torch.autograd.grad(res.dists, (a, b), _d(gd, dev)))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    idx, dists = R.knn_points(p1, p2, l1, l2, norm, K)
    assert torch.equal(out[1][1].cpu(), torch.from_numpy(idx)) and torch.equal(out[1][0].cpu(), torch.from_numpy(dists))
    # the backward of both routes on an idx with entries outside [0, P2): skipped by both, as by the restatement
    bad = R.spoil_idx(rng, idx, P2)[0]
    args = (_d(p1, dev), _d(p2, dev), _d(l1, dev), _d(l2, dev), _d(bad, dev), norm, _d(gd, dev))
    want = R.knn_backward(p1, p2, l1, l2, bad, norm, gd)[:2]
    for x, y, w in zip(B.knn_points_backward(*args), M._knn_torch_backward(*args), want):
        assert torch.equal(x, y) and torch.equal(x.cpu().double(), torch.from_numpy(w))


# ---- chamfer_distance

def test_chamfer_distance_on_two_samplings_of_a_sphere(dev, B):
    rng = np.random.default_rng(21)
    x, y = R.normal(rng, (2000, 3)), R.normal(rng, (2000, 3))
    x, y = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)
    for norm in (1, 2):
        a, b = _d(x, dev, grad=True), _d(y, dev, grad=True)
        cx, cy = maths.chamfer_distance(a, b, norm=norm)
        assert cx.shape == (2000,) and cy.shape == (2000,)
        d64 = R.pair_dists64(x, y, norm)
        for got, want in ((cx, d64.min(1)), (cy, d64.min(0))):
            assert np.all(np.abs(got.detach().cpu().numpy() - want) <= R.dist_bound(3, want))
        # backward() reaches both clouds: each direction moves every query point and no point that is nobody's neighbour (norm 2: exactly
        # the neighbours).  The two directions are taken apart: summed, the +-g of norm 1 can cancel in a point that is query and neighbour.
        for c, q, p in ((cx, a, b), (cy, b, a)):
            gq, gp = torch.autograd.grad(c.mean(), (q, p), retain_graph=True)
            hit = torch.zeros(2000, dtype=torch.bool, device=dev)
            hit[maths.knn_points(q.detach()[None], p.detach()[None], norm=norm).idx.view(-1)] = True
            assert torch.isfinite(gq).all() and torch.isfinite(gp).all() and (gq.abs().sum(1) > 0).all()
            moved = gp.abs().sum(1) > 0                             # norm 1: two queries on opposite sides of a neighbour cancel
            assert moved.any() and not (moved & ~hit).any() and (norm == 1 or torch.equal(moved, hit))
        (cx.mean() + cy.mean()).backward()
        assert a.grad.abs().sum() > 0 and b.grad.abs().sum() > 0
    bx, by = maths.chamfer_distance(_d(x[None], dev), _d(y[None], dev))
    assert bx.shape == (1, 2000) and by.shape == (1, 2000)
