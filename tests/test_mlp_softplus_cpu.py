"""CPU: host side of the softplus hidden activation of the fused decoder (include/nr3d_hip.h NR3D_MLP_ACT_SOFTPLUS, ABI 19) -- the
constants, the size queries (host arithmetic of csrc/mlp_plan.h / mlp_act.h, no kernel runs) and the module's choice of route."""
import ctypes as C

import pytest
import torch

QUERIES = ["nr3d_mlp_packed_floats", "nr3d_mlp_backward_packed_floats", "nr3d_mlp_half_packed_bytes",
           "nr3d_mlp_half_backward_packed_bytes"]
DIMS = [[35, 64, 1], [32, 64, 64, 16], [3, 8, 1], [16, 32, 32, 32, 7], [35, 40, 1], [32, 96, 96, 4], [64, 64, 64, 64], [32, 128, 128, 16],
        [32, 32, 64]]


def _sizes(dims, hidden, out, beta=None):
    from nr3d_lib_amd import _hip as H
    from nr3d_lib_amd.bindings import _mlp
    c = _mlp._CDesc()
    c.n_layers = len(dims) - 1
    for i, d in enumerate(dims):
        c.dims[i] = d
    c.hidden_activation, c.output_activation = hidden, out
    if beta is not None:
        c.softplus_beta = beta
    return [int(getattr(H.lib(), q)(C.byref(c))) for q in QUERIES]


def test_abi_constants():
    from nr3d_lib_amd import _abi
    from nr3d_lib_amd.bindings import _mlp
    assert _mlp.ACT_SOFTPLUS == 2 and (_mlp.ACT_NONE, _mlp.ACT_RELU) == (0, 1)
    assert _abi.ABI_VERSION >= 19
    assert _mlp._CDesc._fields_[-1][0] == "softplus_beta" and C.sizeof(_mlp._CDesc) == 4 * (1 + 9 + 2 + 1)


@pytest.mark.parametrize("dims", DIMS)
def test_softplus_sizes_are_the_relu_sizes(dims):
    """no extra buffers: a valid softplus desc has the four sizes of the same dims with ReLU (0 where ReLU has 0)"""
    from nr3d_lib_amd.bindings import _mlp
    relu = _sizes(dims, _mlp.ACT_RELU, _mlp.ACT_NONE)
    assert relu[0] > 0
    assert _sizes(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_NONE, 100.0) == relu
    assert _sizes(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_RELU, 5.0) == _sizes(dims, _mlp.ACT_RELU, _mlp.ACT_RELU)
    d = _mlp.MLPDesc(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_NONE, beta=100.0)
    assert [d.packed_floats, d.backward_floats, d.half_packed_bytes, d.half_backward_bytes] == relu and d.beta == 100.0


@pytest.mark.parametrize("dims", DIMS[:3])
def test_invalid_softplus_descs_have_size_zero(dims):
    from nr3d_lib_amd.bindings import _mlp
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        assert _sizes(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_NONE, beta) == [0, 0, 0, 0], beta
    # softplus is a hidden activation only
    assert _sizes(dims, _mlp.ACT_RELU, _mlp.ACT_SOFTPLUS, 100.0) == [0, 0, 0, 0]
    assert _sizes(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_SOFTPLUS, 100.0) == [0, 0, 0, 0]
    d = _mlp.MLPDesc(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_NONE, beta=0.0)
    assert not d.fusable and not d.half_fusable and not d.backward_fusable


def test_relu_desc_that_never_touches_the_new_field():
    """a zero-initialised desc with ReLU / none and softplus_beta untouched gives the sizes it gave before the field existed: every 37th
    net of tests/golden/mlp_plan_sizes.npz (recorded from the library long before ABI 19), exact -- and garbage in the field changes
    nothing for ReLU"""
    import os

    import numpy as np
    from nr3d_lib_amd.bindings import _mlp
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_plan_sizes.npz"))
    assert [str(q) for q in gold["queries"]] == QUERIES
    for row, want in list(zip(gold["nets"], gold["sizes"]))[::37]:
        dims = [int(v) for v in row[1:2 + int(row[0])]]
        assert _sizes(dims, _mlp.ACT_RELU, _mlp.ACT_NONE) == [int(v) for v in want], dims
        assert _sizes(dims, _mlp.ACT_RELU, _mlp.ACT_NONE, float("nan")) == [int(v) for v in want], dims


def test_second_order_is_not_fused_for_softplus():
    from nr3d_lib_amd.bindings import _mlp
    for dims in ([35, 64, 1], [16, 32, 32, 4], [32, 64, 64, 16]):
        assert _mlp.MLPDesc(dims, _mlp.ACT_RELU, _mlp.ACT_NONE).second_order_fusable
        sp = _mlp.MLPDesc(dims, _mlp.ACT_SOFTPLUS, _mlp.ACT_NONE, beta=100.0)
        assert sp.backward_fusable and sp.half_backward_fusable and not sp.second_order_fusable


def test_module_maps_softplus_to_the_fused_desc():
    """beta >= FUSED_SOFTPLUS_MIN_BETA with the default threshold fuses; beta = 1, another threshold, mixed betas and a softplus
    output stay on the torch path, which computes torch's softplus"""
    from nr3d_lib_amd.bindings import _mlp
    from nr3d_lib_amd.models.blocks import MLP
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    assert mlp_mod.FUSED_SOFTPLUS_MIN_BETA == 5.0
    for beta, fused in ((100.0, True), (5.0, True), (4.99, False), (1.0, False)):
        m = MLP(35, 1, D=1, W=64, activation={'type': 'softplus', 'beta': beta}, dtype=torch.float)
        d = m.fused_desc()
        assert (d is not None) == fused, beta
        if fused:
            assert d.hidden_activation == _mlp.ACT_SOFTPLUS and d.output_activation == _mlp.ACT_NONE and d.beta == beta
    assert MLP(35, 1, D=1, W=64, activation={'type': 'softplus', 'beta': 100., 'threshold': 10}, dtype=torch.float).fused_desc() is None
    assert MLP(35, 1, D=1, W=64, activation='relu', output_activation={'type': 'softplus', 'beta': 100.}, dtype=torch.float).fused_desc() is None
    mixed = MLP(16, 1, D=2, W=32, activation={'type': 'softplus', 'beta': 100.}, dtype=torch.float)
    mixed.layers[1].activation = torch.nn.Softplus(beta=50.)
    assert mixed.fused_desc() is None
    half = MLP(35, 1, D=1, W=64, activation={'type': 'softplus', 'beta': 100.}, dtype=torch.half)
    assert half.fused_desc() is not None and half.fused_desc().half_backward_fusable
    # the layer-by-layer path (what a CPU tensor takes) is torch's softplus
    m = MLP(6, 2, D=1, W=8, activation={'type': 'softplus', 'beta': 100.}, dtype=torch.float)
    x = torch.randn(5, 6)
    want = torch.nn.functional.linear(torch.nn.functional.softplus(torch.nn.functional.linear(x, m.layers[0].weight, m.layers[0].bias), 100., 20.),
                                      m.layers[1].weight, m.layers[1].bias)
    torch.testing.assert_close(m(x), want)


def test_half_reference_is_stable_under_one_half_rounding():
    """The half GPU test holds EVERY row of dL/dx to 2^-7 of scale although at beta = 100 a unit within ~0.02 of zero has a steep
    derivative.  The reference itself must leave room for that: for the very nets and inputs of test_half_softplus_forward_backward
    (weights from a CPU generator), the rounded-contract fp64 reference evaluated with an extra half rounding of the hidden
    pre-activations goes through the GPU test's own row judge (tests/mlp_half_ref.py assert_rows: softplus has no kink, so no row is
    excused) against the contract without it.  Measured: 0 rows off in each of the six cases ([35, 64, 1], [32, 64, 64, 16],
    [32, 32, 32, 32, 16] x n = 1031, 33) -- half's spacing near zero is far finer than the 0.02 window; the earlier share bound, a
    quarter of the former 2 % cap, is kept beside it"""
    from mlp_half_ref import assert_rows, half_contract
    from test_mlp_softplus_gpu import HALF_DIMS, HALF_NS, half_inputs, half_net
    cpu = torch.device("cpu")
    tol = 2.0 ** -7
    for dims in HALF_DIMS:
        m = half_net(dims, cpu)
        for n in HALF_NS:
            x, gy = half_inputs(dims, n, cpu)
            a, b = half_contract(m, x, gy), half_contract(m, x, gy, round_pre=True)
            bad = ((a[1] - b[1]).abs().amax(1) > tol * float(a[1].abs().max()))
            print(f"{dims} n={n}: {int(bad.sum())} rows")
            assert float(bad.float().mean()) <= 0.005, f"{dims} n={n}: {int(bad.sum())} of {n} rows move under one half rounding"
            assert assert_rows(f"{dims} n={n} round_pre", b[1], m, x, gy, tol, max_excused=0, contract=a) == []
