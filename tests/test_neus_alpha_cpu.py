"""CPU: the host side of the fused NeuS opacity (bindings._neus_alpha, graphics/neus/neus_utils.py FUSED_SDF_TO_ALPHA) -- no kernel
runs: the ABI table, the binding's argument checks, the chain on CPU tensors, and the restatement the GPU tests measure against
(tests/neus_alpha_ref.py) on the reference's recorded values."""
import json
import os

import pytest
import torch

import neus_alpha_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_has_the_entry_points():
    from nr3d_lib_amd import _abi
    assert _abi.ABI_VERSION >= 23
    head = ['int', 'uint32_t', 'uint64_t', 'uint32_t', 'ptr', 'ptr', 'int', 'ptr', 'float', 'ptr', 'int']
    assert _abi.SIGNATURES['nr3d_neus_alpha_fwd'] == ('int', head + ['ptr', 'ptr'])
    assert _abi.SIGNATURES['nr3d_neus_alpha_bwd'] == ('int', head + ['ptr', 'ptr', 'ptr', 'ptr', 'ptr', 'uint64_t', 'ptr'])
    assert _abi.SIGNATURES['nr3d_neus_alpha_bwd_workspace_bytes'] == ('uint64_t', ['int', 'uint32_t', 'uint64_t'])


def test_binding_refuses_before_any_launch():
    """CPU tensors, wrong dtypes and wrong shapes raise from the argument checks (nothing here could launch: there is no GPU)"""
    from nr3d_lib_amd.bindings import _neus_alpha as B
    sdf = torch.zeros(4, 8)
    for call in (lambda: B.sdf_to_alpha_forward(sdf, 64.0),
                 lambda: B.sdf_to_alpha_backward(sdf, 64.0, torch.zeros(4, 7)),
                 lambda: B.sdf_to_alpha_forward(sdf.flatten(), 64.0, torch.tensor([[0, 32]]))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(RuntimeError, match="must be a tensor"):
        B.sdf_to_alpha_forward([0.0, 1.0], 64.0)
    # dtype, shape and contiguity: on "meta" tensors (no data, nothing can launch), with the device check -- covered above -- let through
    def on_meta(*shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device="meta")

    real_require = B.H.require_gpu
    B.H.require_gpu = lambda *a: None
    try:
        with pytest.raises(RuntimeError, match="`sdf` must be float32"):
            B.sdf_to_alpha_forward(on_meta(4, 8, dtype=torch.float16), 64.0)
        with pytest.raises(RuntimeError, match="`sdf` must be float32"):
            B.sdf_to_alpha_forward(on_meta(4, 8, dtype=torch.float64), 64.0)
        with pytest.raises(RuntimeError, match=r"n >= 1"):
            B.sdf_to_alpha_forward(on_meta(4, 0), 64.0)
        with pytest.raises(RuntimeError, match=r"packed `sdf` must be \[S\]"):
            B.sdf_to_alpha_forward(on_meta(4, 8), 64.0, on_meta(4, 2, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="`pack_infos` must be int64"):
            B.sdf_to_alpha_forward(on_meta(32), 64.0, on_meta(4, 2, dtype=torch.int32))
        with pytest.raises(RuntimeError, match=r"`pack_infos` must be \[P, 2\]"):
            B.sdf_to_alpha_forward(on_meta(32), 64.0, on_meta(4, 3, dtype=torch.int64))
        with pytest.raises(RuntimeError, match=r"`pack_sdf_appends` must be \[4\]"):
            B.sdf_to_alpha_forward(on_meta(32), 64.0, on_meta(4, 2, dtype=torch.int64), pack_sdf_appends=on_meta(5))
        with pytest.raises(RuntimeError, match="`pack_sdf_appends` goes with `pack_infos`"):
            B.sdf_to_alpha_forward(on_meta(4, 8), 64.0, pack_sdf_appends=on_meta(4))
        with pytest.raises(RuntimeError, match="`inv_s` must hold one element"):
            B.sdf_to_alpha_forward(on_meta(4, 8), on_meta(2))
        with pytest.raises(RuntimeError, match="`inv_s` must be float32"):
            B.sdf_to_alpha_forward(on_meta(4, 8), on_meta(1, dtype=torch.float64))
        with pytest.raises(RuntimeError, match=r"`grad_alpha` must be \[4, 7\]"):
            B.sdf_to_alpha_backward(on_meta(4, 8), 64.0, on_meta(4, 8))
        with pytest.raises(RuntimeError, match=r"`grad_alpha` must be \[4, 8\]"):
            B.sdf_to_alpha_backward(on_meta(4, 8), 64.0, on_meta(4, 7), append_cdf_1=True)
        with pytest.raises(RuntimeError, match="`grad_alpha` must be float32"):
            B.sdf_to_alpha_backward(on_meta(32), 64.0, on_meta(32, dtype=torch.float16), on_meta(4, 2, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="must be contiguous"):
            B.sdf_to_alpha_forward(on_meta(8, 4).t(), 64.0)
    finally:
        B.H.require_gpu = real_require


@pytest.mark.parametrize("append", [False, True])
def test_cpu_tensors_take_the_chain_bit_for_bit(append):
    """with the switch on, CPU tensors still run the reference's chain: the same bits as fused=False, gradients included"""
    from nr3d_lib_amd.graphics.neus import neus_utils as nu
    assert isinstance(nu.FUSED_SDF_TO_ALPHA, bool)
    saved = nu.FUSED_SDF_TO_ALPHA
    nu.FUSED_SDF_TO_ALPHA = True
    try:
        sdf, g = ref.rows("noisy", 0, 5, 17)
        for inv_s in (64.0, torch.tensor(64.0), torch.tensor(64.0, requires_grad=True)):
            a = sdf.clone().requires_grad_(True)
            b = sdf.clone().requires_grad_(True)
            on = nu.neus_ray_sdf_to_alpha(a, inv_s, append_cdf_1=append)
            off = nu.neus_ray_sdf_to_alpha(b, inv_s, append_cdf_1=append, fused=False)
            assert type(on.grad_fn).__name__ != "_SdfToAlphaBackward"
            assert torch.equal(on, off)
            gg = g if append else g[:, :-1]
            on.backward(gg)
            off.backward(gg)
            assert torch.equal(a.grad, b.grad)
        # the packed helpers reach HIP pack ops on any route and have no CPU form; the row helper on top of the alpha does
        assert torch.equal(nu.neus_ray_sdf_to_vw(sdf, 64.0, append_cdf_1=append),
                           nu.ray_alpha_to_vw(nu.neus_ray_sdf_to_alpha(sdf, 64.0, append_cdf_1=append, fused=False)))
    finally:
        nu.FUSED_SDF_TO_ALPHA = saved


def test_restatement_reproduces_the_recorded_reference_values():
    z = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_samplers.json")))
    sdf, inv_s = torch.tensor(z["sdf"]), z["inv_s"]
    for dtype in (torch.float32, torch.float64):
        got = ref.chain(sdf, inv_s, dtype=dtype)["alpha"].float()
        torch.testing.assert_close(got, torch.tensor(z["neus"]["ray_sdf_to_alpha"]))
        got = ref.chain(sdf, inv_s, append_cdf_1=True, dtype=dtype)["alpha"].float()
        torch.testing.assert_close(got, torch.tensor(z["neus"]["ray_sdf_to_alpha_append"]))
    # ... and, as packs, the project's own chain: rows are packs that tile the buffer
    from nr3d_lib_amd.graphics.neus import neus_utils as nu
    R, n = sdf.shape
    pi = ref.row_pack_infos(R, n, sdf.device)
    for append in (False, True):
        rows = nu.neus_ray_sdf_to_alpha(sdf, inv_s, append_cdf_1=append, fused=False)
        packed = ref.chain(sdf.flatten(), inv_s, pack_infos=pi, append_cdf_1=append, dtype=torch.float32)["alpha"].reshape(R, n)
        assert torch.equal(packed if append else packed[:, :-1], rows)
        assert append or bool((packed[:, -1] == 0).all())


def test_restatement_gradients_and_T():
    """the helper's autograd against the project's chain on the CPU (rows, float32: the same ops, the same bits), and T against a loop"""
    from nr3d_lib_amd.graphics.neus import neus_utils as nu
    sdf, g = ref.rows("noisy", 1, 3, 9)
    for append in (False, True):
        x = sdf.clone().requires_grad_(True)
        s = torch.tensor(20.0, requires_grad=True)
        gg = g if append else g[:, :-1]
        nu.neus_ray_sdf_to_alpha(x, s, append_cdf_1=append, fused=False).backward(gg)
        r = ref.chain(sdf, 20.0, g, append_cdf_1=append, dtype=torch.float32)
        torch.testing.assert_close(r["g_sdf"], x.grad, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(r["g_inv_s"], s.grad, rtol=1e-4, atol=1e-6)
        T = 0.0
        c = torch.sigmoid(sdf.double() * 20.0)
        for row in range(3):
            for i in range(9 if append else 8):
                ci = float(c[row, i])
                cn, xn = (float(c[row, i + 1]), float(sdf[row, i + 1])) if i < 8 else (1.0, 0.0)
                if (ci - cn) / (ci + 1e-5) < 0:
                    continue
                T += abs(float(g[row, i])) * ((cn + 1e-5) / (ci + 1e-5) ** 2 * abs(ci * (1 - ci) * float(sdf[row, i]))
                                              + 1 / (ci + 1e-5) * abs(cn * (1 - cn) * xn))
        assert abs(r["T"] - T) <= 1e-9 * T


def test_generators_meet_the_input_condition():
    """the GPU tests' inputs: no interval with 0 < |z_i - z_next| < 1e-4 in float64 (an interval that close to a tie could take either
    side of the clamp in float32 and float64); exact ties are wanted ("flat")"""
    for kind in ref.KINDS:
        for seed in (0, 1):
            for layout in ("contiguous", "gaps", "shuffled"):
                sdf, pi, app, _ = ref.packs(kind, seed, layout=layout)
                for inv_s in ref.INV_S:
                    assert ref.near_ties(sdf, inv_s, pi, app) == 0, (kind, seed, layout, inv_s)
            for n in (2, 3, 64, 65, 130):
                sdf, _ = ref.rows(kind, seed, 7, n)
                for inv_s in ref.INV_S:
                    assert ref.near_ties(sdf, inv_s) == 0, (kind, seed, n, inv_s)


@pytest.mark.parametrize("layout", ["contiguous", "gaps", "shuffled"])
def test_double_backward_form_of_the_packs_is_the_chain(layout):
    """what the fused Function differentiates under create_graph on packs (torch ops, no host wait, no pack op) against the
    restatement: alpha and, through autograd, every first-order gradient"""
    from nr3d_lib_amd.graphics.neus import neus_utils as nu
    sdf, pi, app, g = ref.packs("noisy", 0, layout=layout)
    for mode in ("none", "one", "sdf"):
        x, s, a = sdf.clone().requires_grad_(True), torch.tensor(20.0, requires_grad=True), app.clone().requires_grad_(True)
        alpha = nu._packed_sdf_to_alpha_by_index(x, s, pi, mode == "one", a if mode == "sdf" else None)
        r = ref.chain(sdf, 20.0, g, pack_infos=pi, append_cdf_1=mode == "one", appends=app if mode == "sdf" else None, dtype=torch.float32)
        assert torch.equal(alpha.detach(), r["alpha"])
        alpha.backward(g)
        torch.testing.assert_close(x.grad, r["g_sdf"], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(s.grad, r["g_inv_s"], rtol=1e-4, atol=1e-6)
        if mode == "sdf":
            torch.testing.assert_close(a.grad, r["g_appends"], rtol=1e-5, atol=1e-6)
