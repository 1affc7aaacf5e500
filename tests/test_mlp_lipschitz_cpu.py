"""CPU: ``LipshitzMLP`` behind ``get_blocks(..., use_lipshitz=True)`` against recorded results of the reference's class
(tests/golden/ref_lipshitz_mlp.npz, written by tests/golden/make_golden_lipshitz.py), the float64 restatement of the normalisation
(tests/mlp_lipschitz_ref.py) against the torch expression on the lattice, and the C ABI's two new entries in the header and the table.

CPU tensors take the reference's torch chain -- the same torch operations in the same order as the recording -- so outputs and gradients
are compared bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import mlp_lipschitz_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = ("init", "half", "quarter")
CFG = {
    "a": dict(D=2, W=16, activation="relu", output_activation="sigmoid"),
    "b": dict(D=1, W=16, activation=dict(type="softplus", beta=100.0), output_activation=None),
}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_lipshitz_mlp.npz"))


def _state_dict(golden, tag):
    pre = f"{tag}_sd_"
    return {k[len(pre):]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith(pre)}


def _module(golden, tag):
    from nr3d_lib_amd.models.blocks import get_blocks
    torch.manual_seed(1)
    m = get_blocks(5, 3, use_lipshitz=True, c_init_factor=float(golden[f"{tag}_c_init_factor"]), **CFG[tag])
    m.load_state_dict(_state_dict(golden, tag), strict=True)
    return m


def test_get_blocks_returns_a_lipshitz_mlp():
    from nr3d_lib_amd.models.blocks import LipshitzMLP, MLP, get_blocks
    m = get_blocks(8, 3, use_lipshitz=True, D=2, W=16)
    assert isinstance(m, LipshitzMLP) and isinstance(m, MLP)
    assert [tuple(l.weight.shape) for l in m.layers] == [(16, 8), (16, 16), (3, 16)]
    c = m.lipshitz_bound_per_layer
    assert isinstance(c, torch.nn.Parameter) and c.requires_grad and c.dtype == torch.float32 and tuple(c.shape) == (3,)
    assert torch.equal(c.detach(), m.initial_bounds(1.0))
    assert sorted(n for n, _ in m.named_parameters()) == sorted(
        ["lipshitz_bound_per_layer"] + [f"layers.{i}.{p}" for i in range(3) for p in ("weight", "bias")])
    assert tuple(m(torch.randn(4, 8)).shape) == (4, 3)
    y, last = m(torch.randn(4, 8), return_last=True)
    assert tuple(y.shape) == (4, 3) and tuple(last.shape) == (4, 16)
    # the regulariser leaves the bounds out: one norm per weight and bias
    assert tuple(m.get_weight_reg().shape) == (6,)
    assert not isinstance(get_blocks(8, 3, D=2, W=16), LipshitzMLP)


def test_constructor_assertions():
    from nr3d_lib_amd.models.blocks import LipshitzMLP, get_blocks
    with pytest.raises(AssertionError):
        get_blocks(8, 3, use_tcnn_backend=True, use_lipshitz=True, D=2, W=16)
    for bad in (dict(skips=[1]), dict(weight_norm=True), dict(equal_lr=True)):
        with pytest.raises(AssertionError):
            LipshitzMLP(8, 3, D=2, W=16, **bad)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_state_dict_and_initial_bounds(golden, tag):
    m = _module(golden, tag)                                   # (strict=True inside)
    f = float(golden[f"{tag}_c_init_factor"])
    recorded = torch.from_numpy(golden[f"{tag}_sd_lipshitz_bound_per_layer"])
    assert recorded.dtype == torch.float32
    assert torch.equal(m.initial_bounds(f), recorded)
    # ... and the constructor uses exactly that on the weights it drew
    from nr3d_lib_amd.models.blocks import LipshitzMLP
    fresh = LipshitzMLP(5, 3, c_init_factor=f, **CFG[tag])
    assert torch.equal(fresh.lipshitz_bound_per_layer.detach(), fresh.initial_bounds(f))
    assert f == 1.0 or not torch.equal(fresh.initial_bounds(f), fresh.initial_bounds(1.0))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_outputs_and_gradients_equal_the_recording(golden, tag):
    m = _module(golden, tag)
    x0 = torch.from_numpy(golden[f"{tag}_x"])
    scaled = 0
    for phase in PHASES:
        if phase != "init":
            with torch.no_grad():
                m.lipshitz_bound_per_layer.mul_(0.5)
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        bound = m.lipshitz_bound_full()
        (y.sum() + bound).backward()
        k = f"{tag}_{phase}_"
        assert np.array_equal(y.detach().numpy(), golden[k + "y"]), phase
        assert np.array_equal(bound.detach().numpy(), golden[k + "bound"]), phase
        assert np.array_equal(x.grad.numpy(), golden[k + "gx"]), phase
        for name, p in m.named_parameters():
            assert np.array_equal(p.grad.numpy(), golden[k + "g_" + name]), (phase, name)
        for layer, c in zip(m.layers, m.lipshitz_bound_per_layer.detach()):
            w = layer.weight.detach()
            wn = m.normalization(w, torch.nn.functional.softplus(c))
            scaled += int((wn != w).any(dim=1).sum())
            assert phase != "init" or torch.equal(wn, w)       # as constructed the normalisation is the identity
    assert scaled > 0


@pytest.mark.parametrize("cols", R.LATTICE_COLS)
def test_restatement_equals_the_torch_expression_on_the_lattice(cols):
    from nr3d_lib_amd.models.blocks import LipshitzMLP
    m = LipshitzMLP(3, 3, D=1, W=4)
    rng = np.random.default_rng(cols)
    Wn, Gn = R.lattice_layer(rng, 13, cols)
    a = np.abs(Wn.astype(np.float64)).sum(1)
    assert set(a[:6]) == set(R.ABS_SUMS) and (a == R.LATTICE_C).any() and (a == 0).any()
    W = torch.from_numpy(Wn).requires_grad_(True)
    c = torch.tensor(R.LATTICE_C, requires_grad=True)
    Wt = m.normalization(W, torch.nn.functional.softplus(c))
    Wt.backward(torch.from_numpy(Gn))
    want = R.normalize(Wn, R.LATTICE_C)
    dW, dc = R.normalize_backward(Wn, R.LATTICE_C, Gn)
    assert np.array_equal(Wt.detach().numpy().astype(np.float64), want)
    assert np.array_equal(W.grad.numpy().astype(np.float64), dW)
    assert float(c.grad) == dc
    # the restatement's results are float32 (and W~ half) numbers: nothing was rounded on the way
    assert np.array_equal(want, want.astype(np.float16).astype(np.float64)) and np.array_equal(dW, dW.astype(np.float32).astype(np.float64))
    # scaled rows exist and clamped rows pass through bit for bit
    assert (want != Wn).any() and np.array_equal(want[a < R.LATTICE_C], Wn[a < R.LATTICE_C].astype(np.float64))


def test_header_and_table_declare_the_entries():
    from nr3d_lib_amd import _abi
    header = open(os.path.join(ROOT, "include", "nr3d_hip.h")).read()
    assert int(re.search(r"#define\s+NR3D_ABI_VERSION\s+(\d+)", header).group(1)) == 30 == _abi.ABI_VERSION      # additions keep the number
    fwd, bwd = "nr3d_mlp_lipschitz_normalize", "nr3d_mlp_lipschitz_normalize_backward"
    assert re.search(r"\bint\s+" + fwd + r"\s*\(", header) and re.search(r"\bint\s+" + bwd + r"\s*\(", header)
    assert _abi.SIGNATURES[fwd] == ("int", ["uint32_t", "ptr", "ptr", "ptr", "int", "ptr", "ptr", "ptr"])
    assert _abi.SIGNATURES[bwd] == ("int", ["uint32_t", "ptr", "ptr", "ptr", "int", "ptr", "ptr", "ptr", "ptr", "ptr"])


def test_bad_arguments_fail_with_a_message(hiplib):
    """no launch: every check sits in front of it, so this needs no GPU"""
    import ctypes as C
    n = 2
    rows, cols = (C.c_uint32 * n)(4, 4), (C.c_uint32 * n)(4, 4)
    ptrs = (C.c_void_p * n)(0x1000, 0x1000)
    null = (C.c_void_p * n)(0x1000, None)
    fwd, bwd = hiplib.nr3d_mlp_lipschitz_normalize, hiplib.nr3d_mlp_lipschitz_normalize_backward
    cases = [
        (fwd, (0, rows, cols, ptrs, 0, 0x1000, ptrs, None), "n_layers"),
        (fwd, (10, rows, cols, ptrs, 0, 0x1000, ptrs, None), "n_layers"),
        (fwd, (n, (C.c_uint32 * n)(4, 0), cols, ptrs, 0, 0x1000, ptrs, None), "rows and columns"),
        (fwd, (n, rows, (C.c_uint32 * n)(4097, 4), ptrs, 0, 0x1000, ptrs, None), "rows and columns"),
        (fwd, (n, rows, cols, null, 0, 0x1000, ptrs, None), "NULL"),
        (fwd, (n, rows, cols, ptrs, 0, None, ptrs, None), "NULL"),
        (fwd, (n, rows, cols, ptrs, 0, 0x1000, null, None), "NULL"),
        (bwd, (0, rows, cols, ptrs, 0, 0x1000, ptrs, ptrs, 0x1000, None), "n_layers"),
        (bwd, (n, rows, cols, ptrs, 0, 0x1000, null, ptrs, 0x1000, None), "NULL"),
        (bwd, (n, rows, cols, ptrs, 0, 0x1000, ptrs, null, 0x1000, None), "NULL"),
        (bwd, (n, rows, cols, ptrs, 0, 0x1000, ptrs, ptrs, None, None), "NULL"),
    ]
    for fn, args, word in cases:
        assert fn(*args) != 0
        assert word in hiplib.nr3d_last_error().decode(), (word, hiplib.nr3d_last_error())


def test_binding_refuses_cpu_tensors(hiplib):
    from nr3d_lib_amd.bindings import _mlp
    w, c = [torch.zeros(3, 3)], torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _mlp.lipschitz_normalize(w, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _mlp.lipschitz_normalize_backward(w, c, [torch.zeros(3, 3)])
