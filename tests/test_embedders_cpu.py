"""CPU: the embedders' restatement (tests/embedders_ref.py) against scipy, finite differences and the reference's recorded results
(tests/golden/ref_embedders.npz); the generated files; the boundary and the Python surface of the port."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import embedders_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ref_embedders.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------------
def test_restatement_matches_scipy_on_the_sphere():
    """all 64 columns against scipy's complex Y_l^m: m > 0: (-1)^m sqrt(2) Re, m < 0: (-1)^m sqrt(2) Im of Y_l^|m| with the Condon-Shortley
    phase removed (scipy carries it, the closed form's sign is s_m alone), m = 0: Re; <= 1e-12"""
    import scipy.special as sps
    rng = np.random.default_rng(1)
    d = rng.standard_normal((300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    theta, phi = np.arccos(np.clip(d[:, 2], -1, 1)), np.arctan2(d[:, 1], d[:, 0])
    got = R.sh(d, 8)
    for l in range(8):
        for m in range(-l, l + 1):
            a = abs(m)
            if hasattr(sps, "sph_harm_y"):
                yc = sps.sph_harm_y(l, a, theta, phi)
            else:
                yc = sps.sph_harm(a, l, phi, theta)
            yc = yc * (-1) ** a                       # scipy includes the Condon-Shortley phase (-1)^m; K Q e^{i m phi} has none
            want = yc.real if m == 0 else (-1) ** a * np.sqrt(2) * (yc.real if m > 0 else yc.imag)
            err = np.abs(got[:, l * l + l + m] - want).max()
            assert err <= 1e-12, (l, m, err)


def test_restatement_jacobian_matches_central_differences():
    rng = np.random.default_rng(2)
    p = rng.uniform(-1, 1, (200, 3))
    J = R.sh_jacobian(p, 8)
    h = 1e-6
    for d in range(3):
        e = np.zeros(3)
        e[d] = h
        fd = (R.sh(p + e, 8) - R.sh(p - e, 8)) / (2 * h)
        assert np.abs(fd - J[:, d]).max() <= 1e-7, (d, np.abs(fd - J[:, d]).max())
    # the fp32 twin stays within its own rounding of the fp64 values: 16 roundings on the bound polynomial
    M, MJ = R.sh_bound(p, 8)
    Y32, J32 = R.sh_all(p.astype(np.float32), 8, np.float32)
    Y64, J64 = R.sh_all(p.astype(np.float32), 8)
    assert (np.abs(Y32 - Y64) <= 32 * R.EPS * M + 1e-30).all() and (np.abs(J32 - J64) <= 32 * R.EPS * MJ + 1e-30).all()


def test_frequency_restatement_second_order_by_differences():
    """backward = d<g, y>/dx and double backward = d<v, gx>/d(g, x), by central differences of the fp64 forward"""
    rng = np.random.default_rng(3)
    D, n = 3, 4
    x, g, v = rng.uniform(-1, 1, (5, D)), rng.standard_normal((5, R.freq_cols(D, n))), rng.standard_normal((5, D))
    y = R.freq_forward(x, n)
    gx = R.freq_backward(g, y, D, n)
    dg, dx = R.freq_backward_backward(v, g, y, D, n)
    h = 1e-6
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        fd = ((R.freq_forward(x + e, n) - R.freq_forward(x - e, n)) * g).sum(1) / (2 * h)
        assert np.abs(fd - gx[:, d]).max() <= 1e-6
        f2 = ((R.freq_backward(g, R.freq_forward(x + e, n), D, n) - R.freq_backward(g, R.freq_forward(x - e, n), D, n)) * v).sum(1) / (2 * h)
        assert np.abs(f2 - dx[:, d]).max() <= 1e-5
    # <v, gx> is linear in g: its gradient is the coefficient of g
    for c in range(g.shape[1]):
        e = np.zeros_like(g)
        e[:, c] = 1.0
        assert np.allclose((R.freq_backward(e, y, D, n) * v).sum(1), dg[:, c], rtol=0, atol=1e-12)


# ---- 2. the reference's recorded results -------------------------------------------------------------------------------------------------
CASES = [(D, n) for D in (1, 3, 4) for n in (0, 1, 6, 10)]


@pytest.mark.parametrize("D,n", CASES)
def test_restatement_matches_the_reference(gold, D, n):
    """legacy embedder values, nablas and the eikonal gradients within the bounds of the GPU test (c = c_ref: the residual recorded with
    the file; the reference's own autograd rounds like the kernels: cos and sin of an fp32 argument, products, a sum)"""
    k = f"sin_D{D}_n{n}_"
    x, g, c = gold[k + "x"], gold[k + "g"], float(gold["c_ref"]) + 2
    assert gold[k + "y"].shape == (x.shape[0], R.freq_cols(D, n))
    y64 = R.freq_forward(x, n)
    assert (np.abs(gold[k + "y"] - y64) <= R.freq_value_tol(x, n, float(gold["c_ref"])) + 1e-300).all()
    assert np.array_equal(gold[k + "y"][:, :D], x)
    P = R.eikonal_program(x, g, n)
    assert (np.abs(gold[k + "nablas"] - P["n"]) <= R.freq_grad_tol(x, g, n, c, y64)).all()
    tol_dg, tol_dx = R.eikonal_tols(x, g, n, c)
    assert (np.abs(gold[k + "dg"] - P["dg"]) <= tol_dg).all()
    assert (np.abs(gold[k + "dx"] - P["dx"]) <= tol_dx).all()
    if n >= 6:        # the bounds are not vacuous: they are small against the values they guard
        assert np.median(tol_dx / (np.abs(P["dx"]) + 1e-30)) < 1e-2


@pytest.mark.parametrize("D,n", CASES)
def test_ported_torch_modules_reproduce_the_reference_bitwise(gold, D, n):
    from nr3d_lib_amd.models.embedders import get_sinusoidal_embedder
    k = f"sin_D{D}_n{n}_"
    m, C = get_sinusoidal_embedder(n, input_dim=D)
    x = torch.from_numpy(gold[k + "x"]).requires_grad_(True)
    g = torch.from_numpy(gold[k + "g"]).requires_grad_(True)
    y = m(x)
    assert C == y.shape[1] and np.array_equal(y.detach().numpy(), gold[k + "y"])
    nab, = torch.autograd.grad(y, x, g, create_graph=True)
    assert np.array_equal(nab.detach().numpy(), gold[k + "nablas"])


def test_annealed_embedder_and_sh_basis_against_the_reference(gold):
    from nr3d_lib_amd.models.embedders import get_sinusoidal_embedder, AnnealedSinusoidalEmbedder
    m, C = get_sinusoidal_embedder(6, input_dim=3, annealed=True)
    assert isinstance(m, AnnealedSinusoidalEmbedder) and C == 39 and "alpha" in m.state_dict() and "freq_bands" not in m.state_dict()
    x = torch.from_numpy(gold["ann_x"])
    for i, a in enumerate(gold["ann_alphas"]):
        m.set_cosine_easing_window(float(a))
        assert np.array_equal(m(x).numpy(), gold[f"ann_y{i}"]), a
    assert not gold["ann_y0"][:, 3:].any() and np.array_equal(gold["ann_y2"], get_sinusoidal_embedder(6, 3)[0](x).numpy())
    # the reference's eval_sh basis (one-hot coefficients) on unit directions is this basis, band by band (fp32 evaluation there)
    deg = int(gold["sh_degrees"])
    assert deg == 5
    assert np.abs(gold["sh_basis"] - R.sh(gold["sh_dirs"], deg)).max() <= 2e-6


# ---- 3. generated files and the boundary -----------------------------------------------------------------------------------------------
def test_generated_files_are_current():
    for tool in ("gen_sh_basis.py", "gen_abi.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_sh_basis
    finally:
        sys.path.pop(0)
    assert open(os.path.join(ROOT, "nr3d_lib_amd", "csrc", "sh_basis.inc")).read() == gen_sh_basis.render()
    # the tables are the restatement's polynomials, rounded once
    v, z = gen_sh_basis.tables()
    for l in range(8):
        for a in range(l + 1):
            for order, tab in ((0, v), (1, z)):
                want = [c for _, c in R.zpoly(l, a, order)] if a + order <= l else []
                got = tab[l][a][:len(want)]
                assert all(w != 0 for w in want) and not any(tab[l][a][len(want):])
                assert np.array_equal(np.array(got, np.float32), np.array(want, np.float64).astype(np.float32)), (l, a, order)


def test_library_exports_the_embedder_symbols(hiplib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nr3d_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nr3d_(?:sh|freq)_encode_[A-Za-z0-9_]+)\s*\(", header)))
    assert declared == ["nr3d_freq_encode_bwd", "nr3d_freq_encode_bwd_bwd", "nr3d_freq_encode_fwd", "nr3d_sh_encode_bwd", "nr3d_sh_encode_fwd"]
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "nr3d_lib_amd", "libnr3d_hip.so")], capture_output=True,
                        text=True).stdout
    exported = set(re.findall(r" T (nr3d_(?:sh|freq)_encode_[A-Za-z0-9_]+)", nm))
    assert exported == set(declared), exported ^ set(declared)
    from nr3d_lib_amd import _abi
    assert _abi.ABI_VERSION >= 15 and all(s in _abi.SIGNATURES for s in declared)
    # argument checks happen before any launch: no GPU is needed to be refused
    L = hiplib
    assert L.nr3d_sh_encode_fwd(4, 2, 4, 0, None, None, 16, None, None) != 0 and b"3-D" in L.nr3d_last_error()
    assert L.nr3d_sh_encode_fwd(4, 3, 9, 0, None, None, 81, None, None) != 0 and b"[1, 8]" in L.nr3d_last_error()
    assert L.nr3d_sh_encode_fwd(4, 3, 4, 2, None, None, 16, None, None) != 0 and b"dtype" in L.nr3d_last_error()
    assert L.nr3d_sh_encode_fwd(4, 3, 4, 0, None, None, 15, None, None) != 0 and b"y_stride" in L.nr3d_last_error()
    assert L.nr3d_sh_encode_fwd(4, 3, 4, 0, None, None, 16, None, None) != 0 and b"NULL" in L.nr3d_last_error()
    assert L.nr3d_sh_encode_fwd(0, 3, 4, 0, None, None, 16, None, None) == 0
    assert L.nr3d_sh_encode_bwd(0, 3, 4, 0, None, 16, None, None, None, 0, None) == 0
    assert L.nr3d_freq_encode_fwd(4, 3, 6, 38, None, None, 38, None) != 0 and b"expected D + 2 D n_freq = 39" in L.nr3d_last_error()
    assert L.nr3d_freq_encode_fwd(4, 3, 25, 153, None, None, 153, None) != 0 and b"at most 24" in L.nr3d_last_error()
    assert L.nr3d_freq_encode_fwd(4, 0, 1, 0, None, None, 0, None) != 0
    assert L.nr3d_freq_encode_fwd(2 ** 27, 3, 6, 39, None, None, 39, None) != 0 and b"split the batch" in L.nr3d_last_error()
    assert L.nr3d_freq_encode_fwd(0, 3, 6, 39, None, None, 39, None) == 0
    assert L.nr3d_freq_encode_bwd(0, 3, 6, 39, None, None, 39, None, None) == 0
    assert L.nr3d_freq_encode_bwd_bwd(0, 3, 6, 39, None, None, None, 39, None, None, None) == 0
    assert L.nr3d_freq_encode_bwd(4, 3, 6, 39, None, None, 39, None, None) != 0 and b"NULL" in L.nr3d_last_error()


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_binding_twins_surface():
    from nr3d_lib_amd.bindings import _shencoder as S, _freqencoder as F
    assert list(inspect.signature(S.sh_encode_forward).parameters) == ["inputs", "outputs", "B", "D", "C", "calc_grad_inputs", "dy_dx"]
    assert list(inspect.signature(S.sh_encode_backward).parameters) == ["grad", "inputs", "B", "D", "C", "dy_dx", "grad_inputs"]
    assert list(inspect.signature(F.freq_encode_forward).parameters) == ["inputs", "B", "D", "deg", "C", "outputs"]
    assert list(inspect.signature(F.freq_encode_backward).parameters) == ["grad", "outputs", "B", "D", "deg", "C", "grad_inputs"]
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="`inputs` must be a CUDA tensor"):
        S.sh_encode_forward(x, torch.zeros(4, 16), 4, 3, 4, False, torch.zeros(1))
    with pytest.raises(RuntimeError, match="`inputs` must be a CUDA tensor"):
        S.sh_encode_backward(torch.zeros(4, 16), x, 4, 3, 4, None, torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="`inputs` must be a CUDA tensor"):
        F.freq_encode_forward(x, 4, 3, 6, 39, torch.zeros(4, 39))
    with pytest.raises(RuntimeError, match="`grad` must be a CUDA tensor"):
        F.freq_encode_backward(torch.zeros(4, 39), torch.zeros(4, 39), 4, 3, 6, 39, x)


def test_modules_surface():
    import nr3d_lib_amd.models.embedders as E
    from nr3d_lib_amd.models.embedders import spherical_harmonics, sinusoidal_cuda, sinusoidal_pytorch
    assert spherical_harmonics.sphere_harmonics.__all__ == ["sh_encode", "SHEncoder"]
    assert sinusoidal_cuda.freq.__all__ == ["freq_encode", "FreqEncoder"]
    assert sinusoidal_pytorch.__all__ == ["SinusoidalEmbedder", "AnnealedSinusoidalEmbedder", "get_sinusoidal_embedder"]
    assert spherical_harmonics.sphere_harmonics.RECOMPUTE_BACKWARD in (True, False)
    d = inspect.signature(E.SHEncoder.__init__).parameters
    assert (d["input_dim"].default, d["degree"].default) == (3, 4)
    assert E.SHEncoder().out_features == 16 and E.SHEncoder(3, 8).out_features == 64
    for bad in (dict(input_dim=2), dict(degree=0), dict(degree=9)):
        with pytest.raises(AssertionError):
            E.SHEncoder(**bad)
    d = inspect.signature(E.FreqEncoder.__init__).parameters
    assert (d["input_dim"].default, d["n_frequencies"].default, d["include_input"].default) == (3, 4, True)
    assert E.FreqEncoder(3, 10).out_features == 63 and E.FreqEncoder(7, 0).out_features == 7
    with pytest.raises(AssertionError):
        E.FreqEncoder(include_input=False)
    assert list(inspect.signature(E.get_embedder).parameters) == ["embed_cfg", "input_dim", "use_tcnn_backend"]
    cfg = {"type": "spherical", "degree": 4}
    for tp, kw, cls, n_out in (("none", {}, torch.nn.Identity, 5), ("identity", {}, torch.nn.Identity, 5),
                               ("spherical", {"degree": 3}, E.SHEncoder, 9), ("sinusoidal", {"n_frequencies": 6}, E.FreqEncoder, 39),
                               ("sinusoidal_legacy", {"n_frequencies": 6}, E.SinusoidalEmbedder, 39)):
        dim = 5 if cls is torch.nn.Identity else 3
        enc, n = E.get_embedder({"type": tp, **kw}, dim)
        assert isinstance(enc, cls) and n == n_out and enc._embedder_type == tp
    assert E.get_embedder(cfg)[1] == 16 and cfg == {"type": "spherical", "degree": 4}          # the caller's dict is not consumed
    with pytest.raises(RuntimeError, match="Unsupported embeder type=fourier"):
        E.get_embedder({"type": "fourier"})
    with pytest.raises(NotImplementedError):
        E.get_embedder(cfg, 3, use_tcnn_backend=True)
    with pytest.raises(NotImplementedError):
        E.get_embedder({**cfg, "use_tcnn_backend": True})
    # CPU tensors are refused by name
    with pytest.raises(RuntimeError, match="CPU tensor"):
        E.SHEncoder()(torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        E.FreqEncoder()(torch.zeros(2, 3))


def test_mlpnet_is_exported():
    from nr3d_lib_amd.models.blocks import mlp
    import nr3d_lib_amd.models.blocks as blocks
    assert "MLPNet" in mlp.__all__ and blocks.MLPNet is mlp.MLPNet and issubclass(mlp.MLPNet, mlp.MLP)
    d = inspect.signature(mlp.MLPNet.__init__).parameters
    assert d["embed_cfg"].default == {"type": "identity"} and d["D"].default == 4 and d["W"].default == 128
    m = mlp.MLPNet(3, 3, embed_cfg={"type": "sinusoidal_legacy", "n_frequencies": 2}, D=1, W=8)
    assert m.in_features == 15 and m(torch.zeros(4, 3)).shape == (4, 3) and m.embedder._embedder_type == "sinusoidal_legacy"
    assert mlp.MLPNet(3, 3, embed_cfg={"type": "spherical", "degree": 4}, D=1, W=32).in_features == 16
