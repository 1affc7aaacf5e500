"""CPU: the double backward of softplus hidden layers (include/nr3d_hip.h nr3d_mlp_softplus_backward_backward, ABI 21) -- the formulas
the kernel implements (tests/mlp_softplus2_ref.py) against torch's own double backward in float64, and the host side: the ABI table and
the eligibility query (host arithmetic, no kernel runs)."""
import ctypes as C

import pytest
import torch

from mlp_softplus2_ref import make_inputs, make_params, restated, torch_double_backward

# dims, n, bias, beta, output ReLU
CASES = [
    ([35, 64, 1], 257, True, 100.0, False),
    ([16, 32, 32, 32, 7], 257, False, 100.0, False),
    ([32, 64, 16], 257, True, 5.0, False),
    ([3, 8, 1], 1, True, 100.0, False),
    ([16, 32, 32, 4], 257, True, 100.0, False),
    ([18, 64, 3], 257, True, 100.0, True),
]


def _compare(got, ref, tag):
    """(dgy, dx, [dW], [db]) of the restatement against autograd's: <= 1e-12 of each tensor's maximum (observed: <= 1.3e-15)"""
    names = ["dL/d(dL/dy)", "dL/dx"] + [f"dW[{l}]" for l in range(len(ref[2]))] + [f"db[{l}]" for l in range(len(ref[3]))]
    for name, a, b in zip(names, [got[0], got[1], *got[2], *got[3]], [ref[0], ref[1], *ref[2], *ref[3]]):
        assert (a is None) == (b is None), f"{tag} {name}"
        if b is None:
            continue
        assert torch.isfinite(a).all(), f"{tag} {name}"
        scale = float(b.abs().max()) or 1.0
        err = float((a - b).abs().max()) / scale
        print(f"{tag} {name}: {err:.2e}")
        assert err <= 1e-12, f"{tag} {name}: {err:.2e} of the maximum"


@pytest.mark.parametrize("dims,n,bias,beta,out_relu", CASES)
def test_restated_formulas_are_torchs_double_backward(dims, n, bias, beta, out_relu):
    ws, bs = make_params(dims, bias, seed=len(dims) + dims[0])
    x, u, v = make_inputs(dims, n)
    _compare(restated(ws, bs, x, u, v, beta, out_relu), torch_double_backward(ws, bs, x, u, v, beta, out_relu), str(dims))


def test_saturated_units_are_finite_and_equal():
    """x * 40: beta z reaches +-1e4 -- above the threshold s = 1 and e = 0 exactly, far below it s = 0"""
    dims = [32, 64, 64, 16]
    ws, bs = make_params(dims, True, seed=31)
    x, u, v = make_inputs(dims, 257, seed=32, scale=40.0)
    z1 = torch.nn.functional.linear(x.double(), ws[0].double(), bs[0].double())
    assert float(z1.max()) > 100.0 and float(z1.min()) < -100.0
    _compare(restated(ws, bs, x, u, v, 100.0), torch_double_backward(ws, bs, x, u, v, 100.0), "saturated")


def test_new_entry_points_are_in_the_abi_table():
    from nr3d_lib_amd import _abi
    assert _abi.ABI_VERSION >= 21
    assert _abi.SIGNATURES["nr3d_mlp_softplus_backward_backward_ok"] == ("int", ["ptr"])
    assert _abi.SIGNATURES["nr3d_mlp_softplus_backward_backward"] == (
        "int", ["ptr", "uint64_t", "ptr", "int64_t", "int64_t", "ptr", "int64_t", "ptr", "int64_t", "int64_t", "ptr", "ptr", "int64_t",
                "ptr", "int64_t", "int64_t", "ptr", "ptr", "ptr"])


def _ok(dims, hidden, out, beta):
    from nr3d_lib_amd import _hip as H
    from nr3d_lib_amd.bindings import _mlp
    c = _mlp._CDesc()
    c.n_layers = len(dims) - 1
    for i, d in enumerate(dims):
        c.dims[i] = d
    c.hidden_activation, c.output_activation, c.softplus_beta = hidden, out, beta
    return int(H.lib().nr3d_mlp_softplus_backward_backward_ok(C.byref(c)))


def test_eligibility_query():
    from nr3d_lib_amd.bindings import _mlp
    sp, relu, none = _mlp.ACT_SOFTPLUS, _mlp.ACT_RELU, _mlp.ACT_NONE
    # every backward-fusable shape of tests/test_mlp_second_order_cpu.py: softplus with a valid beta, output none or ReLU
    for dims in ((32, 64, 64, 16), (32, 32, 16), (18, 32, 3), (32, 32, 32, 16), (32, 64, 16), (64, 64, 64, 64), (64, 64, 64), (32, 64, 64, 64),
                 (32, 64, 64), (64, 64, 16), (35, 64, 1), (32, 64, 64, 1), (16, 32, 32, 32, 7), (3, 8, 1)):
        assert _ok(dims, sp, none, 100.0) == 1 and _ok(dims, sp, relu, 5.0) == 1, dims
        assert _ok(dims, relu, none, 100.0) == 0 and _ok(dims, none, none, 100.0) == 0, dims
        for beta in (0.0, -1.0, float("nan"), float("inf")):
            assert _ok(dims, sp, none, beta) == 0, (dims, beta)
        assert _ok(dims, sp, sp, 100.0) == 0 and _ok(dims, relu, sp, 100.0) == 0, dims
        d = _mlp.MLPDesc(list(dims), sp, none, beta=100.0)
        assert d.softplus_second_order_fusable and not d.second_order_fusable and d.backward_fusable
        assert not _mlp.MLPDesc(list(dims), relu, none).softplus_second_order_fusable
    # outside the fused backward: hidden width 128, three hidden layers wider than 32, output wider than the hidden layers, one layer
    for dims in ((32, 128, 128, 16), (32, 128, 4), (32, 64, 64, 64, 16), (32, 32, 64), (32, 16)):
        assert _ok(dims, sp, none, 100.0) == 0, dims
        assert not _mlp.MLPDesc(list(dims), sp, none, beta=100.0).softplus_second_order_fusable


def test_the_switch_exists_and_the_old_query_is_unchanged():
    from nr3d_lib_amd.bindings import _mlp
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    assert isinstance(mlp_mod.FUSED_SOFTPLUS_SECOND_ORDER, bool)
    d = _mlp.MLPDesc([35, 64, 1], _mlp.ACT_SOFTPLUS, _mlp.ACT_NONE, beta=100.0)
    assert not d.second_order_fusable and d.softplus_second_order_fusable
    assert callable(_mlp.backward_backward_softplus)
