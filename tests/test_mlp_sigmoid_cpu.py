"""CPU: host side of the sigmoid output activation of the fused decoder (include/nr3d_hip.h NR3D_MLP_ACT_SIGMOID, ABI 22) -- the
constants, the size queries (host arithmetic of csrc/mlp_plan.h / mlp_act.h, no kernel runs), which activation codes are refused, the
module's choice of route, and that the yardstick of the half GPU test can be met by the contract it is measured against."""
import ctypes as C

import pytest
import torch

QUERIES = ["nr3d_mlp_packed_floats", "nr3d_mlp_backward_packed_floats", "nr3d_mlp_half_packed_bytes",
           "nr3d_mlp_half_backward_packed_bytes"]
DIMS = [[32, 64, 64, 3], [35, 64, 1]]


def _cdesc(dims, hidden, out, beta=None):
    from nr3d_lib_amd.bindings import _mlp
    c = _mlp._CDesc()
    c.n_layers = len(dims) - 1
    for i, d in enumerate(dims):
        c.dims[i] = d
    c.hidden_activation, c.output_activation = hidden, out
    if beta is not None:
        c.softplus_beta = beta
    return c


def _sizes(dims, hidden, out, beta=None):
    from nr3d_lib_amd import _hip as H
    c = _cdesc(dims, hidden, out, beta)
    return [int(getattr(H.lib(), q)(C.byref(c))) for q in QUERIES]


def test_abi_constants():
    from nr3d_lib_amd import _abi
    from nr3d_lib_amd.bindings import _mlp
    assert _abi.ABI_VERSION >= 22
    assert _mlp.ACT_SIGMOID == 3 and (_mlp.ACT_NONE, _mlp.ACT_RELU, _mlp.ACT_SOFTPLUS) == (0, 1, 2)
    assert C.sizeof(_mlp._CDesc) == 4 * (1 + 9 + 2 + 1)                     # the struct did not change


@pytest.mark.parametrize("dims", DIMS)
def test_sigmoid_sizes_are_the_relu_output_sizes(dims):
    """no extra buffers: a sigmoid output has the four sizes of the same dims with a ReLU output, with ReLU and with softplus hidden layers"""
    from nr3d_lib_amd.bindings import _mlp
    relu = _sizes(dims, _mlp.ACT_RELU, _mlp.ACT_RELU)
    assert all(v > 0 for v in relu)
    assert _sizes(dims, _mlp.ACT_RELU, _mlp.ACT_SIGMOID) == relu
    assert _sizes(dims, _mlp.ACT_NONE, _mlp.ACT_SIGMOID) == _sizes(dims, _mlp.ACT_NONE, _mlp.ACT_RELU)
    assert _sizes(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_SIGMOID, 100.0) == _sizes(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_RELU, 100.0) == relu
    d = _mlp.MLPDesc(dims, _mlp.ACT_RELU, _mlp.ACT_SIGMOID)
    assert [d.packed_floats, d.backward_floats, d.half_packed_bytes, d.half_backward_bytes] == relu
    assert d.fusable and d.backward_fusable and d.half_fusable and d.half_backward_fusable


@pytest.mark.parametrize("dims", DIMS)
def test_codes_the_kernels_do_not_know_have_size_zero(dims):
    """sigmoid is an output activation only, softplus a hidden one only, and a code outside the enum is refused on either field (it
    used to pass the size queries and run as the identity)"""
    from nr3d_lib_amd.bindings import _mlp
    assert _sizes(dims, _mlp.ACT_SIGMOID, _mlp.ACT_NONE) == [0, 0, 0, 0]
    assert _sizes(dims, _mlp.ACT_SIGMOID, _mlp.ACT_SIGMOID) == [0, 0, 0, 0]
    assert _sizes(dims, _mlp.ACT_RELU, _mlp.ACT_SOFTPLUS, 100.0) == [0, 0, 0, 0]
    for code in (4, 255):
        assert _sizes(dims, code, _mlp.ACT_NONE) == [0, 0, 0, 0], code
        assert _sizes(dims, _mlp.ACT_RELU, code) == [0, 0, 0, 0], code
        assert _sizes(dims, _mlp.ACT_SOFTPLUS, code, 100.0) == [0, 0, 0, 0], code
        assert _sizes(dims, code, _mlp.ACT_SIGMOID) == [0, 0, 0, 0], code
    d = _mlp.MLPDesc(dims, _mlp.ACT_SIGMOID, _mlp.ACT_NONE)
    assert not d.fusable and not d.half_fusable and not d.backward_fusable and not d.half_backward_fusable


@pytest.mark.parametrize("dims", DIMS)
def test_no_double_backward_through_a_sigmoid_output(dims):
    from nr3d_lib_amd import _hip as H
    from nr3d_lib_amd.bindings import _mlp
    for hidden, beta in ((_mlp.ACT_RELU, None), (_mlp.ACT_NONE, None), (_mlp.ACT_SOFTPLUS, 100.0)):
        c = _cdesc(dims, hidden, _mlp.ACT_SIGMOID, beta)
        assert int(H.lib().nr3d_mlp_backward_backward_ok(C.byref(c))) == 0
        assert int(H.lib().nr3d_mlp_softplus_backward_backward_ok(C.byref(c))) == 0
        d = _mlp.MLPDesc(dims, hidden, _mlp.ACT_SIGMOID, beta=beta or 1.0)
        assert d.backward_fusable and not d.second_order_fusable and not d.softplus_second_order_fusable
    # the twins keep theirs
    assert _mlp.MLPDesc(dims, _mlp.ACT_RELU, _mlp.ACT_RELU).second_order_fusable
    assert _mlp.MLPDesc(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_NONE, beta=100.0).softplus_second_order_fusable


def test_module_maps_sigmoid_to_the_fused_desc():
    from nr3d_lib_amd.bindings import _mlp
    from nr3d_lib_amd.models.blocks import MLP, get_blocks
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    kw = dict(D=2, W=64, activation='relu', output_activation='sigmoid')
    for extra in (dict(), dict(dtype=torch.half), dict(activation={'type': 'softplus', 'beta': 100.})):
        d = MLP(32, 3, **{**kw, **extra}).fused_desc()
        assert d is not None and d.output_activation == _mlp.ACT_SIGMOID, extra
        assert d.hidden_activation == (_mlp.ACT_SOFTPLUS if 'activation' in extra else _mlp.ACT_RELU)
        assert not mlp_mod._fused_second_order(d)
    assert MLP(32, 3, **{**kw, 'activation': 'sigmoid'}).fused_desc() is None
    assert MLP(32, 3, **{**kw, 'activation': 'sigmoid', 'output_activation': None}).fused_desc() is None
    assert MLP(32, 3, skips=[1], **kw).fused_desc() is None
    d = get_blocks(32, 3, **kw).fused_desc()
    assert d is not None and d.output_activation == _mlp.ACT_SIGMOID
    # the layer-by-layer path (what a CPU tensor takes) and the differentiable re-evaluation's activation are torch's sigmoid
    m = MLP(6, 2, D=1, W=8, activation='relu', output_activation='sigmoid')
    x = torch.randn(5, 6)
    z = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(x, m.layers[0].weight, m.layers[0].bias)), m.layers[1].weight,
                                   m.layers[1].bias)
    torch.testing.assert_close(m(x), torch.sigmoid(z))
    assert torch.equal(mlp_mod._torch_activation(z, m.fused_desc(), hidden=False), torch.sigmoid(z))
    assert torch.equal(mlp_mod._torch_activation(z, m.fused_desc(), hidden=True), torch.relu(z))


def test_half_yardstick_is_reachable():
    """The half GPU test measures the kernels against the half contract with the sigmoid on the UNROUNDED output accumulator, holds the
    rows of dL/dx to 2^-7 of scale (a row off it must be proven to sit on a ReLU kink) and y to 2^-9.  For the very inputs of test_half_sigmoid_forward_backward, in fp64:
    the contract in both orders at the output (sigmoid on the accumulator, then one rounding / round, sigmoid, round -- what a separate
    pass over a half tensor computes) and the network without any rounding.  Rows of dL/dx that differ by more than the tolerance between
    the two orders: none, so the order is no source of misses; between either order and the unrounded network -- what half rounding as
    such moves --: below the cap.  Measured here (dims, n: rows between the orders, rows against the unrounded network for the
    accumulator / the rounded order, largest difference of y between the orders as a fraction of scale):
      [32, 64, 64, 3] 4099: 0, 0.88 % / 0.88 %, 4.9e-4      [31, 64, 3] 257: 0, 0.39 % / 0.39 %, 5.0e-4
      [16, 32, 32, 32, 3] 513: 0, 0.58 % / 0.58 %, 4.9e-4    [64, 64, 64, 64] 1031: 0, 1.45 % / 1.45 %, 4.9e-4      [3, 8, 1] 1: 0, 0 / 0, 0
    (half_net draws the weights from a CPU generator: these are the GPU test's nets)."""
    from mlp_half_ref import half_contract
    from test_mlp_sigmoid_gpu import HALF_CASES, half_inputs, half_net
    cpu = torch.device("cpu")
    tol = 2.0 ** -7

    def rows(a, b):
        return float(((a - b).abs().amax(1) > tol * float(b.abs().max())).float().mean())
    for dims, n in HALF_CASES:
        m = half_net(dims, cpu)
        x, gy = half_inputs(dims, n, cpu)
        acc, rounded, exact = (half_contract(m, x, gy, order=o) for o in ("accumulator", "rounded", "unrounded"))
        between = rows(acc[1], rounded[1])
        off = rows(acc[1], exact[1]), rows(rounded[1], exact[1])
        dy = float((acc[0] - rounded[0]).abs().max() / acc[0].abs().max())
        print(f"{dims} n={n}: dL_dx rows between the orders {between:.4f}, against the unrounded network {off[0]:.4f} / {off[1]:.4f}; "
              f"y between the orders {dy:.2e}")
        assert between == 0.0, f"{dims} n={n}: {between:.4f} of the dL/dx rows depend on the order at the output"
        assert max(off) < 0.02, f"{dims} n={n}: {max(off):.4f} of the dL/dx rows move under half rounding alone"
        assert dy <= 2.0 ** -9, f"{dims} n={n}: y differs by {dy:.2e} of scale between the two orders"
