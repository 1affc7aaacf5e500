"""CPU: the row judge of tests/mlp_half_ref.py (assert_rows) catches what the rule it replaces -- "at most 2 % of the dL/dx rows miss
2^-7 of scale" -- let pass.  A small model of the half kernels of csrc/mlp_half.hip stands in for them: fp32 linear layers on the
half-rounded operands, every layer's output rounded to half, dL/d(pre-activation) rounded to half between the layers, a ReLU unit on
where its rounded output is not zero.  Nets and inputs are those of the GPU tests (weights from a CPU generator, 0.4 / 0.2 randn)."""
import pytest
import torch

from mlp_half_ref import assert_rows, fill_parameters, flip_band, half_contract, max_excused

N = 4099                                     # sixteen workgroups of 256 samples and a partial tile of 3
TOL = 2.0 ** -7
SOFTPLUS = dict(type="softplus", beta=100.0)
NETS = {
    "relu": ([32, 64, 64, 16], "relu", None),
    "relu_out": ([64, 48, 64, 8], "relu", "relu"),
    "softplus": ([32, 64, 64, 16], SOFTPLUS, None),
}


def _net(dims, hidden, out, seed=0):
    from nr3d_lib_amd.models.blocks import MLP
    m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation=hidden, output_activation=out, bias=True, dtype=torch.half,
            device=torch.device("cpu"))
    return fill_parameters(m, seed)


def _inputs(dims, n=N):
    g = torch.Generator(device="cpu").manual_seed(1)
    return torch.randn(n, dims[0], generator=g), torch.randn(n, dims[-1], generator=g)


def kernel_model(m, x, gy, z0_shift=None):
    """dL/dx of the kernel model, fp32.  z0_shift = (unit, delta): delta is added to that unit's layer-0 bias after its rounding"""
    rnd = lambda t: t.detach().half().float()
    with torch.no_grad():
        h, saved = rnd(x), []
        for i, l in enumerate(m.layers):
            z = torch.nn.functional.linear(h, rnd(l.weight), None if l.bias is None else rnd(l.bias))
            if i == 0 and z0_shift is not None:
                z[:, z0_shift[0]] += z0_shift[1]
            a = l.activation
            if a is None:
                h, d = rnd(z), torch.ones_like(z)
            elif isinstance(a, torch.nn.ReLU):
                h = rnd(torch.relu(z))
                d = (h != 0).float()
            elif isinstance(a, torch.nn.Softplus):
                h, d = rnd(torch.nn.functional.softplus(z, a.beta, a.threshold)), torch.sigmoid(a.beta * z)
            else:
                assert isinstance(a, torch.nn.Sigmoid)
                s = torch.sigmoid(z)
                h, d = rnd(s), s * (1 - s)
            saved.append((rnd(l.weight), d))
        g = rnd(gy)
        for W, d in reversed(saved):
            g = rnd(g * d) @ W
    return g


def _old_rule_passes(got, dx64):
    """the replaced assertion, verbatim"""
    bad = ((got.double() - dx64).abs().amax(1) > TOL * float(dx64.abs().max()))
    return float(bad.float().mean()) <= 0.02


_cases = {}


def _case(name):
    """net, inputs, the model's dL/dx and the contract's, computed once per net"""
    if name not in _cases:
        dims, hidden, out = NETS[name]
        m = _net(dims, hidden, out)
        x, gy = _inputs(dims)
        _cases[name] = (m, x, gy, kernel_model(m, x, gy), half_contract(m, x, gy)[1])
    return _cases[name]


@pytest.mark.parametrize("name", list(NETS))
def test_the_kernel_model_passes_with_a_quarter_of_the_cap(name):
    """the cap on excused rows must not be eaten by rounding that the contract allows: the model needs at most a quarter of it (here
    none: max_excused(4099) = 2)"""
    m, x, gy, got, _ = _case(name)
    excused = assert_rows(name, got, m, x, gy, TOL, max_excused=max_excused(N))
    assert len(excused) <= max_excused(N) // 4


def _plant(fault, got):
    got = got.clone()
    if fault == "neighbour":                      # row 63 of every 64 carries its neighbour's gradient: one sample per two tiles
        got[63::64] = got[62::64]
    elif fault == "edge_zero":                    # the last row of every workgroup of 256 is never written
        got[255::256] = 0
    elif fault == "nan":
        got[1234] = float("nan")
    else:
        assert fault == "column"                  # one column scaled in every 40th row
        got[::40, 3] *= 1.5
    return got


@pytest.mark.parametrize("fault", ["neighbour", "edge_zero", "nan", "column"])
@pytest.mark.parametrize("name", list(NETS))
def test_planted_faults_fail(name, fault):
    """each planted fault makes assert_rows raise -- with the whole cap to spend -- and the first three passed the rule it replaces
    (NaN compares false, and 1 / 64 or 1 / 256 of the rows is below 2 %)"""
    m, x, gy, got, dx64 = _case(name)
    bad = _plant(fault, got)
    if fault != "column":
        assert _old_rule_passes(bad, dx64), "the fault is meant to be one the old rule let pass"
    with pytest.raises(AssertionError) as e:
        assert_rows(f"{name} {fault}", bad, m, x, gy, TOL, max_excused=max_excused(N))
    print(e.value)
    if fault == "nan":
        assert "not finite" in str(e.value)
    else:
        assert "r % 32" in str(e.value) and "r % 256" in str(e.value)


@pytest.mark.parametrize("name", ["relu", "relu_out"])
def test_a_true_flip_is_excused(name):
    """a kink built by hand: row R is one-hot and unit U's layer-0 bias cancels its only product exactly, so the contract's z is 0 (unit
    off); the model's bias is shifted by half the unit's band, so the model, and only it, switches the unit on.  The row misses the
    plain tolerance and is reported as excused by exactly that unit"""
    R, U, J = 1000, 5, 7
    dims, hidden, out = NETS[name]
    m = _net(dims, hidden, out)
    x, gy = _inputs(dims)
    with torch.no_grad():
        x[R] = 0
        x[R, J] = 1.0
        m.layers[0].weight[U] *= 8.0                  # an exact scaling of the unit's weights, so that switching it moves the row by more than the tolerance
        m.layers[0].bias[U] = -m.layers[0].weight[U, J].half().float()
    _, dx64, _, _, zs = half_contract(m, x, gy)
    band = float(flip_band(m, x)[0][R, U])
    assert float(zs[0][R, U]) == 0.0 and band > 0
    got = kernel_model(m, x, gy, z0_shift=(U, 0.5 * band))
    assert float((got[R].double() - dx64[R]).abs().max()) > TOL * float(dx64.abs().max()), "the flip is meant to move the row"
    plain = kernel_model(m, x, gy)
    assert float((plain[R].double() - dx64[R]).abs().max()) <= TOL * float(dx64.abs().max())
    excused = assert_rows(name, got, m, x, gy, TOL, max_excused=max_excused(N))
    assert excused == [(R, ((0, U),))]
    with pytest.raises(AssertionError, match="more than 0"):            # ... and an excused row still counts against the cap
        assert_rows(name, got, m, x, gy, TOL, max_excused=0)
    # a near unit is no licence: the same row scaled by 1.25 is explained by no pattern of its near units
    wrong = got.clone()
    wrong[R] = plain[R] * 1.25
    with pytest.raises(AssertionError, match=f"row {R} .*near units: layer 0 unit {U}"):
        assert_rows(name, wrong, m, x, gy, TOL, max_excused=max_excused(N))


def test_forced_masks_reproduce_the_free_pattern():
    """half_contract with masks = its own on / off pattern is half_contract without masks"""
    m, x, gy, _, _ = _case("relu_out")
    free = half_contract(m, x[:300], gy[:300])
    forced = half_contract(m, x[:300], gy[:300], masks=[z > 0 for z in free[4]])
    assert len(free[4]) == 3
    for a, b in zip(free[:2], forced[:2]):
        assert torch.equal(a, b)


# one small case through the three former copies of the contract (tests/test_mlp_gpu.py _half_reference, test_mlp_softplus_gpu.py and
# test_mlp_sigmoid_gpu.py half_reference), recorded before they were removed: sum_i t_i cos(i) over the flattened y, dL/dx and the
# concatenated dW / db, in fp64
FORMER = {
    ("relu", ()): (0.13670081841439047, 0.6191018420622401, 4.360977424948591),
    ("softplus", ()): (0.395580181697438, 0.1085723940875074, 30.119058481009276),
    ("softplus", (("round_pre", True),)): (0.395580181697438, 0.10857363022871713, 30.119198858772723),
    ("sigmoid", (("order", "accumulator"),)): (0.8840566094128155, 0.10573918765670558, 7.080794613695177),
    ("sigmoid", (("order", "rounded"),)): (0.8834585260384347, 0.10571928748387245, 7.080859095783579),
    ("sigmoid", (("order", "unrounded"),)): (0.8838137370726292, 0.10588753668799827, 7.081400846934372),
}


def _former_case(hidden, out):
    from nr3d_lib_amd.models.blocks import MLP
    m = MLP(5, 3, D=2, W=[8, 8], activation=hidden, output_activation=out, bias=True, dtype=torch.half, device=torch.device("cpu"))
    fill_parameters(m, 77)
    g = torch.Generator(device="cpu").manual_seed(78)
    return m, torch.randn(7, 5, generator=g), torch.randn(7, 3, generator=g)


def _checksums(r):
    def cs(t):
        t = t.double().flatten()
        return float((t * torch.cos(torch.arange(t.numel(), dtype=torch.float64))).sum())
    return cs(r[0]), cs(r[1]), cs(torch.cat([w.flatten() for w in r[2]] + [b.flatten() for b in r[3]]))


@pytest.mark.parametrize("key", list(FORMER))
def test_half_contract_equals_the_former_copies(key):
    net, kw = key
    hidden, out = {"relu": ("relu", "relu"), "softplus": (SOFTPLUS, None), "sigmoid": ("relu", "sigmoid")}[net]
    m, x, gy = _former_case(hidden, out)
    got = _checksums(half_contract(m, x, gy, **dict(kw)))
    assert got == pytest.approx(FORMER[key], rel=1e-12, abs=1e-13)
