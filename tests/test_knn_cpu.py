"""CPU: the k-NN contract (include/nr3d_hip.h: nr3d_knn_points) in its numpy restatement tests/knn_ref.py, and the pure-torch route of
``nr3d_lib_amd.maths`` (``knn_points``, ``knn_gather``, ``chamfer_distance`` on CPU tensors) against the restatement and against the
recorded results of the reference's Python layer (tests/golden/ref_knn.npz).  On lattice inputs everything is exact."""
import os
import re

import numpy as np
import pytest
import torch

import knn_ref as R
from nr3d_lib_amd import maths
from nr3d_lib_amd.maths import pytorch3d_knn as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_knn.npz")


def _t(a, **kw):
    return torch.from_numpy(np.ascontiguousarray(a)).requires_grad_(kw.get("grad", False))


# ---- the restatement itself

def test_ref_known_answers():
    p1 = np.array([[[0.0], [1.0], [5.0]]], np.float32)
    p2 = np.array([[[1.0], [0.0], [1.0], [4.0]]], np.float32)
    idx, d = R.knn_points(p1, p2, K=3)
    # ties by ascending j: for the query 1.0, j = 0 before j = 2; for 0.0 at distance 1, j = 0 before j = 2
    assert idx.tolist() == [[[1, 0, 2], [0, 2, 1], [3, 0, 2]]]
    assert d.tolist() == [[[0.0, 1.0, 1.0], [0.0, 0.0, 1.0], [1.0, 16.0, 16.0]]]
    idx, d = R.knn_points(p1, p2, K=2, norm=1)
    assert idx.tolist() == [[[1, 0], [0, 2], [3, 0]]] and d.tolist() == [[[0.0, 1.0], [0.0, 0.0], [1.0, 4.0]]]
    # at the K-th place the lower index wins; padding: lengths2 < K, rows past lengths1
    idx, d = R.knn_points(p1, p2, lengths1=[2], lengths2=[3], K=4)
    assert idx.tolist() == [[[1, 0, 2, 0], [0, 2, 1, 0], [0, 0, 0, 0]]]
    assert d.tolist() == [[[0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]]]
    # 3-4-5 in two dimensions
    idx, d = R.knn_points(np.zeros((1, 1, 2), np.float32), np.array([[[3.0, 4.0], [-1.0, 0.0]]], np.float32), K=2)
    assert idx.tolist() == [[[1, 0]]] and d.tolist() == [[[1.0, 25.0]]]
    g1, g2 = R.knn_backward(np.zeros((1, 1, 2)), np.array([[[3.0, 4.0], [-1.0, 0.0]]]), None, None, idx, 2, np.array([[[1.0, 0.5]]]))[:2]
    assert g1.tolist() == [[[2.0 * 1.0 - 3.0, -4.0]]] and g2.tolist() == [[[3.0, 4.0], [-2.0, 0.0]]]


@pytest.mark.parametrize("norm", [1, 2])
def test_ref_against_topk_without_ties(norm):
    rng = np.random.default_rng(1)
    p1, p2 = R.normal(rng, (2, 40, 3)), R.normal(rng, (2, 55, 3))
    idx, d = R.knn_points(p1, p2, norm=norm, K=6)
    for n in range(2):
        dm = torch.from_numpy(R.pair_dists(p1[n], p2[n], norm))
        assert len(np.unique(dm.numpy())) == dm.numel()            # tie-free
        v, i = torch.topk(dm, 6, dim=1, largest=False, sorted=True)
        assert np.array_equal(i.numpy(), idx[n]) and np.array_equal(v.numpy(), d[n])
        assert np.all(np.abs(d[n].astype(np.float64) - np.take_along_axis(R.pair_dists64(p1[n], p2[n], norm), idx[n], 1))
                      <= R.dist_bound(3, d[n].astype(np.float64)))


def test_lattice_is_exact():
    rng = np.random.default_rng(2)
    for D in (1, 3, 8, 9):
        a, b = R.lattice(rng, (2000, D)), R.lattice(rng, (2000, D))
        assert D * (2 * R.lattice_kmax(D)) ** 2 <= 2 ** 24 < D * (4 * R.lattice_kmax(D)) ** 2
        d64 = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum(-1)
        d32 = np.zeros(2000, np.float32)
        for c in range(D):                                         # separate multiply and add
            d32 = (d32 + ((a[:, c] - b[:, c]) * (a[:, c] - b[:, c])).astype(np.float32)).astype(np.float32)
        chain = np.array([R.pair_dists(a[i:i + 1], b[i:i + 1], 2)[0, 0] for i in range(0, 2000, 50)])
        assert np.array_equal(d32.astype(np.float64), d64) and np.array_equal(chain.astype(np.float64), d64[::50])


# ---- the CPU route against the restatement and the golden file

@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_cpu_route_equals_reference_wrapper(golden, tag):
    g = {k[2:]: golden[k] for k in golden.files if k.startswith(tag + "_")}
    p1, p2 = _t(g["p1"], grad=True), _t(g["p2"], grad=True)
    l1, l2 = _t(golden["lengths1"]), _t(golden["lengths2"])
    res = maths.knn_points(p1, p2, l1, l2, norm=int(g["norm"]), K=int(g["K"]), return_nn=True)
    assert isinstance(res, M._KNN) and res._fields == ("dists", "idx", "knn")
    assert res.idx.dtype == torch.int64 and not res.idx.requires_grad
    assert np.array_equal(res.dists.detach().numpy(), g["dists"]) and np.array_equal(res.idx.numpy(), g["idx"])
    assert np.array_equal(res.knn.detach().numpy(), g["knn"])
    assert np.array_equal(maths.knn_gather(p2.detach(), res.idx, l2).numpy(), g["knn"])
    g1, g2 = torch.autograd.grad(res.dists, (p1, p2), _t(g["grad_dists"]))
    assert np.array_equal(g1.numpy(), g["grad_p1"]) and np.array_equal(g2.numpy(), g["grad_p2"])
    # return_sorted=False and version are accepted and change nothing
    again = maths.knn_points(p1, p2, l1, l2, norm=int(g["norm"]), K=int(g["K"]), version=3, return_sorted=False)
    assert torch.equal(again.dists, res.dists) and torch.equal(again.idx, res.idx) and again.knn is None


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K,P1,P2", [(1, 1, 5, 1), (3, 4, 70, 33), (3, 40, 9, 31), (9, 17, 11, 64), (2, 8, 130, 7)])
def test_cpu_route_equals_restatement_on_the_lattice(monkeypatch, norm, D, K, P1, P2):
    monkeypatch.setattr(M, "CHUNK_BYTES", 4 * P2 * 3 * 16)         # several chunks
    rng = np.random.default_rng(D * 100 + K)
    p1, p2 = R.lattice(rng, (3, P1, D), kmax=4), R.lattice(rng, (3, P2, D), kmax=4)
    l1, l2 = np.array([0, P1 // 2, P1]), np.array([min(2, P2), P2, 0])
    gd = (2.0 ** rng.integers(-2, 3, size=(3, P1, K))).astype(np.float32)
    for lens in ((None, None), (l1, l2)):
        a, b = _t(p1, grad=True), _t(p2, grad=True)
        res = maths.knn_points(a, b, *(None if l is None else _t(l) for l in lens), norm=norm, K=K, return_nn=True)
        idx, d = R.knn_points(p1, p2, *lens, norm=norm, K=K)
        assert np.array_equal(res.idx.numpy(), idx) and np.array_equal(res.dists.detach().numpy(), d)
        assert np.array_equal(res.knn.detach().numpy(), R.knn_gather(p2, idx, lens[1]))
        g1, g2 = torch.autograd.grad(res.dists, (a, b), _t(gd))
        w1, w2 = R.knn_backward(p1, p2, *lens, idx, norm, gd)[:2]
        assert np.array_equal(g1.numpy().astype(np.float64), w1) and np.array_equal(g2.numpy().astype(np.float64), w2)


@pytest.mark.parametrize("norm", [1, 2])
def test_backward_agrees_with_float64_autograd_of_the_dense_formula(norm):
    rng = np.random.default_rng(7)
    p1, p2 = R.normal(rng, (2, 30, 3)), R.normal(rng, (2, 41, 3))
    gd = R.normal(rng, (2, 30, 4))
    a, b = _t(p1, grad=True), _t(p2, grad=True)
    res = maths.knn_points(a, b, norm=norm, K=4)
    g1, g2 = torch.autograd.grad(res.dists, (a, b), _t(gd))
    a64, b64 = _t(p1.astype(np.float64), grad=True), _t(p2.astype(np.float64), grad=True)
    diff = a64[:, :, None, :] - b64[:, None, :, :]
    dm = (diff * diff).sum(-1) if norm == 2 else diff.abs().sum(-1)
    picked = torch.gather(dm, 2, res.idx)
    assert np.all(np.abs(picked.detach().numpy() - res.dists.detach().numpy()) <= R.dist_bound(3, picked.detach().numpy()))
    w1, w2 = torch.autograd.grad(picked, (a64, b64), _t(gd.astype(np.float64)))
    _, _, s1, s2, m2 = R.knn_backward(p1, p2, None, None, res.idx.numpy(), norm, gd)
    assert np.all(np.abs(g1.numpy() - w1.numpy()) <= (4 + 3) * R.EPS * s1)
    assert np.all(np.abs(g2.numpy() - w2.numpy()) <= (m2[..., None] + 3) * R.EPS * s2)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K", [(3, 4), (3, 33)])
def test_cpu_route_clamps_lengths_outside_the_cloud(norm, D, K):
    """"a value of lengths outside [0, P] is clamped into it": -5, -1, P + 1, 2^40, INT64_MIN and INT64_MAX in both lengths, forward
    and backward, against the restatement with its np.clip (the GPU twin: test_lengths_outside_the_cloud_are_clamped)"""
    N, P1, P2 = 16, 70, 7
    rng = np.random.default_rng(N + K)
    p1, p2 = R.lattice(rng, (N, P1, D), kmax=8), R.lattice(rng, (N, P2, D), kmax=8)
    l1, l2 = R.wild_lengths(rng, N, P1), R.wild_lengths(rng, N, P2, at=8)
    assert {-5, -1, P1 + 1, 2 ** 40, R.I64_MIN, R.I64_MAX} <= set(l1.tolist()) and {-5, -1, P2 + 1, 2 ** 40, R.I64_MIN, R.I64_MAX} <= set(l2.tolist())
    gd = (2.0 ** rng.integers(-2, 3, size=(N, P1, K))).astype(np.float32)
    a, b = _t(p1, grad=True), _t(p2, grad=True)
    res = maths.knn_points(a, b, _t(l1), _t(l2), norm=norm, K=K)
    idx, d = R.knn_points(p1, p2, l1, l2, norm=norm, K=K)
    assert idx.any() and np.array_equal(res.idx.numpy(), idx) and np.array_equal(res.dists.detach().numpy(), d)
    # every wild value is what its clamped value is
    i2, d2 = R.knn_points(p1, p2, np.clip(l1, 0, P1), np.clip(l2, 0, P2), norm=norm, K=K)
    assert np.array_equal(i2, idx) and np.array_equal(d2, d)
    g1, g2 = torch.autograd.grad(res.dists, (a, b), _t(gd))
    w1, w2 = R.knn_backward(p1, p2, l1, l2, idx, norm, gd)[:2]
    assert w1.any() and np.array_equal(g1.numpy().astype(np.float64), w1) and np.array_equal(g2.numpy().astype(np.float64), w2)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D,K", [(3, 8), (9, 3)])
def test_cpu_route_backward_skips_idx_outside_the_cloud(norm, D, K):
    """"an idx outside [0, P2) is skipped": a tenth of a real forward's idx overwritten by -1, P2, P2 + 7 and 2^40; those (n, i, k)
    terms are missing from both gradients, the others are as before (the GPU twin: test_backward_skips_idx_outside_the_cloud)"""
    N, P1, P2 = 2, 300, 5
    rng = np.random.default_rng(D + K)
    p1, p2 = R.lattice(rng, (N, P1, D), kmax=8), R.lattice(rng, (N, P2, D), kmax=8)
    gd = (2.0 ** rng.integers(-2, 3, size=(N, P1, K))).astype(np.float32)
    for lens in ((None, None), (np.array([299, 120]), np.array([5, 2]))):
        idx = R.knn_points(p1, p2, lens[0], lens[1], norm, K)[0]
        bad, hit = R.spoil_idx(rng, idx, P2)
        assert all((bad == v).any() for v in (-1, P2, P2 + 7, 2 ** 40)) and np.array_equal(bad[~hit], idx[~hit])
        full = [torch.full((N,), P, dtype=torch.int64) if l is None else _t(l) for l, P in zip(lens, (P1, P2))]
        g1, g2 = M._knn_torch_backward(_t(p1), _t(p2), *full, _t(bad), norm, _t(gd))
        w1, w2 = R.knn_backward(p1, p2, lens[0], lens[1], bad, norm, gd)[:2]
        clean = R.knn_backward(p1, p2, lens[0], lens[1], idx, norm, gd)[:2]
        assert not np.array_equal(w1, clean[0]) and not np.array_equal(w2, clean[1])
        assert np.array_equal(g1.numpy().astype(np.float64), w1) and np.array_equal(g2.numpy().astype(np.float64), w2)


def test_ref_backward_skips_idx_outside_the_cloud():
    """the restatement itself, on the 3-4-5 answer of test_ref_known_answers: a spoiled slot takes its term out of both gradients"""
    p1, p2 = np.zeros((1, 1, 2)), np.array([[[3.0, 4.0], [-1.0, 0.0]]])
    for j in (-1, 2, 9, 2 ** 40):
        g1, g2 = R.knn_backward(p1, p2, None, None, np.array([[[1, j]]]), 2, np.array([[[1.0, 0.5]]]))[:2]
        assert g1.tolist() == [[[2.0, 0.0]]] and g2.tolist() == [[[0.0, 0.0], [-2.0, 0.0]]]


def test_knn_gather_edges():
    x = torch.arange(24, dtype=torch.float32).view(2, 4, 3)
    idx = torch.tensor([[[0, 3, 1]], [[2, 0, 0]]])
    out = maths.knn_gather(x, idx, torch.tensor([4, 1]))
    assert out.shape == (2, 1, 3, 3)
    assert torch.equal(out[0, 0], x[0][[0, 3, 1]]) and torch.equal(out[1, 0, 0], x[1, 2]) and not out[1, 0, 1:].any()
    assert torch.equal(maths.knn_gather(x, idx), torch.stack([x[0][idx[0]], x[1][idx[1]]]))
    assert torch.equal(maths.knn_gather(torch.zeros(2, 0, 5), torch.zeros(2, 3, 2, dtype=torch.int64)), torch.zeros(2, 3, 2, 5))
    with pytest.raises(ValueError, match="batch"):
        maths.knn_gather(x, idx[:1])


def test_empty_clouds():
    for shape1, shape2 in (((0, 4, 3), (0, 5, 3)), ((2, 0, 3), (2, 5, 3)), ((2, 4, 3), (2, 0, 3))):
        a, b = torch.zeros(shape1, requires_grad=True), torch.zeros(shape2, requires_grad=True)
        res = maths.knn_points(a, b, K=2, return_nn=True)
        assert res.dists.shape == (shape1[0], shape1[1], 2) and not res.dists.any() and not res.idx.any()
        assert res.knn.shape == (shape1[0], shape1[1], 2, 3) and not res.knn.any()
        g1, g2 = torch.autograd.grad(res.dists.sum(), (a, b))
        assert g1.shape == a.shape and g2.shape == b.shape and not g1.any() and not g2.any()


# ---- the surface

def test_header_and_table_have_the_entries():
    from nr3d_lib_amd import _abi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nr3d_hip.h")).read(), flags=re.S)
    want = {"nr3d_knn_points": 13, "nr3d_knn_points_backward": 15, "nr3d_knn_fast_path": 2, "nr3d_knn_tile_points": 1,
            "nr3d_knn_launch_plan": 4}
    for name, nargs in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        ret, args = _abi.SIGNATURES[name]
        assert ret == "int" and len(args) == nargs, (name, args)
    assert _abi.SIGNATURES["nr3d_knn_points"][1][:4] == ["ptr"] * 4 and _abi.SIGNATURES["nr3d_knn_points"][1][4:7] == ["uint64_t"] * 3
    assert _abi.SIGNATURES["nr3d_knn_launch_plan"][1] == ["uint64_t", "uint64_t", "uint32_t", "uint32_t"]
    assert _abi.ABI_VERSION == 30


def test_launch_plan_is_the_documented_rule(hiplib):
    """launch_plan (the function the launcher calls) against the rule as DESIGN.md 4h words it: the wide variant (R = 4 for KB 1, 2 for
    KB 4 .. 16, none for KB 32; 256 lanes) when N ceil(P1 / (256 R)) >= 512 workgroups, else R = 1 and the workgroup halved down to
    one wave while there are fewer than 512; nothing for a (D, K) off the fast kernel.  No device is touched."""
    from nr3d_lib_amd.bindings import _pytorch3d_knn as B

    def rule(N, P1, K):
        Rw = 4 if K == 1 else 2 if K <= 16 else 1
        if Rw > 1 and N * -(-P1 // (256 * Rw)) >= 512:
            return Rw, 256
        wg = 256
        while wg > 64 and N * -(-P1 // wg) < 512:
            wg //= 2
        return 1, wg

    seen = set()
    for N in (1, 2, 3, 255, 256, 257, 300, 511, 512, 513, 1 << 20):
        for P1 in (1, 64, 65, 128, 129, 200, 256, 257, 300, 512, 513, 1000, 1024, 1025, 2049, 1 << 20):
            for K in (1, 2, 4, 5, 8, 9, 16, 17, 32):
                for D in (1, 3, 8):
                    assert B.launch_plan(N, P1, D, K) == rule(N, P1, K), (N, P1, D, K)
                seen.add(rule(N, P1, K))
            assert B.launch_plan(N, P1, 9, 1) is None and B.launch_plan(N, P1, 3, 33) is None and B.launch_plan(N, P1, 0, 1) is None
    assert seen == {(1, 64), (1, 128), (1, 256), (2, 256), (4, 256)}
    assert B.launch_plan(2 ** 31 - 1, 2 ** 31 - 1, 3, 1) == (4, 256)


def test_every_compiled_kernel_has_a_named_case(hiplib):
    """tests/test_knn_gpu.py's coverage(): every instantiation of csrc/knn.hip -- k_knn<D, KB, NORM, 1> (80), the wide k_knn<D, KB, NORM,
    R> (64: R = 4 for KB 1, 2 for KB 4, 8, 16) and k_knn_any<DC> (9) -- is claimed by at least one case; the case exists under that
    id, and the launcher's own plan for the case's rows is the variant it claims, so a retuned kWantGroups or Wide<KB>::R fails here
    (and in the case itself) instead of silently moving the coverage"""
    import test_knn_gpu as G
    from nr3d_lib_amd.bindings import _pytorch3d_knn as B
    table = G.coverage()
    narrow = {("k_knn", D, KB, norm, 1) for D in range(1, 9) for KB in (1, 4, 8, 16, 32) for norm in (1, 2)}
    wide = {("k_knn", D, KB, norm, 4 if KB == 1 else 2) for D in range(1, 9) for KB in (1, 4, 8, 16) for norm in (1, 2)}
    generic = {("k_knn_any", DC) for DC in range(9)}
    assert (len(narrow), len(wide), len(generic)) == (80, 64, 9)
    assert set(table) == narrow | wide | generic
    for inst, cases in table.items():
        assert cases, inst
        for case, N, P1, D, K in cases:
            name, params = re.fullmatch(r"(\w+)\[([\d-]+)\]", case).groups()
            marks = [m for m in getattr(G, name).pytestmark if m.name == "parametrize"]
            assert len(marks) == 1 and marks[0].args[0] == "D,K,norm" and tuple(int(p) for p in params.split("-")) in marks[0].args[1], case
            assert (D, K) == tuple(int(p) for p in params.split("-"))[:2]
            plan = B.launch_plan(N, P1, D, K)
            if inst[0] == "k_knn":
                assert B.fast_path(D, K) and D == inst[1] and G.bucket(K) == inst[2] and plan is not None and plan[0] == inst[4], (inst, case)
                assert inst[3] == int(params.split("-")[2])
            else:
                assert plan is None and not B.fast_path(D, K) and inst[1] == (D if D <= 8 else 0), (inst, case)


def test_module_surface():
    import inspect
    assert M.__all__ == ["knn_points", "knn_gather"]
    assert list(inspect.signature(M.knn_points).parameters) == ["p1", "p2", "lengths1", "lengths2", "norm", "K", "version", "return_nn",
                                                                "return_sorted"]
    assert list(inspect.signature(M.knn_gather).parameters) == ["x", "idx", "lengths"]
    sig = inspect.signature(maths.chamfer_distance)
    assert list(sig.parameters) == ["x", "y", "norm", "backend"] and sig.parameters["backend"].default == "pt3d"
    assert M.FUSED_KNN in (True, False) and isinstance(M.GENERIC_MIN_ROWS, int) and M.GENERIC_MIN_ROWS >= 0
    assert not M._fused(torch.zeros(1, 4, 3), 1) and not M._fused(torch.zeros(1, 4, 3))      # CPU tensors: the torch route
    from nr3d_lib_amd.bindings import _pytorch3d_knn as B
    assert callable(B.knn_points_idx) and callable(B.knn_points_backward) and callable(B.TILE) and callable(B.fast_path)
    assert callable(B.launch_plan) and "launch_plan" in B.__all__


def test_argument_errors():
    a, b = torch.zeros(2, 4, 3), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="batch"):
        maths.knn_points(a, b[:1])
    with pytest.raises(ValueError, match="point dimension"):
        maths.knn_points(a, torch.zeros(2, 5, 2))
    with pytest.raises(ValueError, match="1 or 2 norm"):
        maths.knn_points(a, b, norm=3)
    with pytest.raises(RuntimeError, match="float32"):
        maths.knn_points(a.double(), b.double())
    with pytest.raises(RuntimeError, match="float32"):
        maths.knn_points(a, b.half())
    with pytest.raises(RuntimeError, match="K = 0"):
        maths.knn_points(a, b, K=0)
    with pytest.raises(RuntimeError, match="lengths1"):
        maths.knn_points(a, b, lengths1=torch.tensor([4, 4], dtype=torch.int32))
    with pytest.raises(ValueError, match="1 or 2 norm"):
        maths.chamfer_distance(a, b, norm=3)
    with pytest.raises(ValueError, match="batch and point dimensions"):
        maths.chamfer_distance(a, b[:1])
    with pytest.raises(RuntimeError, match="unknown backend"):
        maths.chamfer_distance(a, b, backend="nope")
    from nr3d_lib_amd.bindings import _pytorch3d_knn as B
    with pytest.raises(RuntimeError, match="GPU only|CPU tensor"):
        B.knn_points_idx(a, b, None, None, 2, 1, -1)
    with pytest.raises(RuntimeError, match="float32"):
        B.knn_points_idx(a.double(), b.double(), None, None, 2, 1, -1)


# ---- chamfer_distance

@pytest.mark.parametrize("norm", [1, 2])
def test_chamfer_distance_2d_and_3d_inputs(norm):
    rng = np.random.default_rng(11)
    x, y = R.lattice(rng, (2, 37, 3), kmax=8), R.lattice(rng, (2, 50, 3), kmax=8)
    cx, cy = maths.chamfer_distance(_t(x), _t(y), norm=norm)
    assert cx.shape == (2, 37) and cy.shape == (2, 50)
    assert np.array_equal(cx.numpy(), R.knn_points(x, y, norm=norm)[1][..., 0]) and np.array_equal(cy.numpy(), R.knn_points(y, x, norm=norm)[1][..., 0])
    c0, c1 = maths.chamfer_distance(_t(x[1]), _t(y[1]), norm=norm)
    assert c0.shape == (37,) and c1.shape == (50,) and torch.equal(c0, cx[1]) and torch.equal(c1, cy[1])


def test_chamfer_backends():
    rng = np.random.default_rng(12)
    x, y = R.lattice(rng, (2, 37, 3), kmax=8), R.lattice(rng, (2, 50, 3), kmax=8)
    a = maths.chamfer_distance(_t(x), _t(y))
    b = maths.chamfer_distance(_t(x), _t(y), backend="pytorch")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])         # x against Y: the reference's typo is not reproduced
    b = maths.chamfer_distance(_t(x[0]), _t(y[0]), backend="pytorch")
    assert torch.equal(a[0][0], b[0]) and torch.equal(a[1][0], b[1])
    with pytest.raises(AssertionError, match="norm 2 only"):
        maths.chamfer_distance(_t(x), _t(y), norm=1, backend="pytorch")
    try:
        import pytorch3d  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            maths.chamfer_distance(_t(x), _t(y), backend="pt3d_import")
    xg, yg = _t(x, grad=True), _t(y, grad=True)
    cx, cy = maths.chamfer_distance(xg, yg)
    (cx.mean() + cy.mean()).backward()
    assert xg.grad.abs().sum() > 0 and yg.grad.abs().sum() > 0
