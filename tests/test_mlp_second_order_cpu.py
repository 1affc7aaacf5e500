"""CPU: host logic of the fused double backward (csrc/mlp.hip nr3d_mlp_backward_backward_ok), no kernel runs."""
from nr3d_lib_amd.bindings import _mlp


def test_second_order_fusable_follows_the_fused_backward():
    """the double backward runs on every shape the fused backward runs on (same LDS plan), and on no other"""
    for dims in ((32, 64, 64, 16), (32, 32, 16), (18, 32, 3), (32, 32, 32, 16), (32, 64, 16), (64, 64, 64, 64), (64, 64, 64), (32, 64, 64, 64),
                 (32, 64, 64), (64, 64, 16), (35, 64, 1), (32, 64, 64, 1), (16, 32, 32, 32, 7), (3, 8, 1)):
        for act in (_mlp.ACT_RELU, _mlp.ACT_NONE):
            d = _mlp.MLPDesc(list(dims), act, _mlp.ACT_NONE)
            assert d.backward_fusable and d.second_order_fusable, dims
    # hidden width above 64, three hidden layers wider than 32, output wider than the hidden layers, widths above 128, one layer
    for dims in ((32, 128, 128, 16), (32, 64, 64, 64, 16), (32, 32, 64), (32, 256, 1), (32, 16)):
        d = _mlp.MLPDesc(list(dims), 1, 0)
        assert not d.backward_fusable and not d.second_order_fusable, dims


def test_new_entry_points_are_in_the_abi_table():
    from nr3d_lib_amd import _abi
    assert _abi.ABI_VERSION >= 10
    assert _abi.SIGNATURES["nr3d_mlp_backward_backward_ok"] == ("int", ["ptr"])
    assert _abi.SIGNATURES["nr3d_mlp_backward_backward"] == (
        "int", ["ptr", "uint64_t", "ptr", "int64_t", "int64_t", "ptr", "int64_t", "ptr", "int64_t", "int64_t", "ptr", "ptr", "int64_t",
                "ptr", "ptr"])
