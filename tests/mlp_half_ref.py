"""The half contract of the fused MLP kernels (csrc/mlp_half.hip) in fp64, and a judge for the rows of dL/dx -- plain torch, for CPU
and GPU tensors alike; shared by tests/test_mlp_gpu.py, test_mlp_softplus_gpu.py, test_mlp_sigmoid_gpu.py and their CPU companions.

The contract: weights, biases, x and dL/dy rounded to half; every layer's output (after its activation) rounded to half, straight
through for the gradient; everything in between exact (fp64).  The kernels differ from it by fp32 accumulation, by the odd activation
that rounds the other way after it, and by rounding dL/d(pre-activation) to half between the layers: 2^-7 of the scale of dL/dx covers
that -- EXCEPT in a row where a ReLU unit's pre-activation sits so close to zero that the kernel and the contract switch the unit
differently; there a whole weight path enters or leaves the row's gradient.  assert_rows() accepts such a row only after it has
PROVEN the kink: the contract, re-evaluated on that row with a few of its near-zero units switched the other way, must give the
kernel's gradient within the same 2^-7.  Nothing else excuses a row, and a network without ReLU layers has no excuse at all."""
import itertools

import torch

MAX_FLIP_UNITS = 8                 # a row's near units that may be switched: the 8 with the smallest |z| (255 patterns at the most)


def _kind(layer):
    a = layer.activation
    if a is None:
        return "none"
    if isinstance(a, torch.nn.ReLU):
        return "relu"
    if isinstance(a, torch.nn.Sigmoid):
        return "sigmoid"
    assert isinstance(a, torch.nn.Softplus), a
    return "softplus"


def _activate(layer, z):
    k = _kind(layer)
    if k == "none":
        return z
    if k == "sigmoid":
        return torch.sigmoid(z)
    if k == "softplus":
        return torch.nn.functional.softplus(z, layer.activation.beta, layer.activation.threshold)
    return torch.relu(z)


class _Round(torch.autograd.Function):
    """round to half, straight through for the gradient"""
    @staticmethod
    def forward(ctx, t):
        return t.half().double()

    @staticmethod
    def backward(ctx, g):
        return g


def fill_parameters(m, seed, weight_scale=0.4, bias_scale=0.2):
    """randn parameters from a CPU generator, copied in: the same net on every device and machine -> m"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (weight_scale if p.dim() > 1 else bias_scale)).to(p.device))
    return m


def max_excused(n):
    """how many rows of n a test may excuse by a proven kink.  A condition, not a measurement: a CPU model of the kernels (fp32
    accumulation, half outputs, half dL/dz) needs 2 rows of 200 001 on the 32 -> 64 -> 64 -> 16 net and none on smaller cases"""
    return max(2, n // 2000)


def half_contract(m, x, gy, round_pre=False, order="accumulator", masks=None):
    """-> (y, dx, [dW], [db | None], zs) as fp64 tensors; zs: the pre-activations of every ReLU layer (a ReLU output layer included).

    round_pre: the pre-activations of the hidden layers that have an activation are rounded to half as well (a sensitivity probe; the
    kernels do not do that).
    order, at the output layer: "accumulator": the activation on the unrounded accumulator, then one rounding -- what the kernels do;
    "rounded": the accumulator rounded to half first, then the activation, then rounded (a separate pass over a half tensor);
    "unrounded": nothing is rounded, neither the layers' outputs nor the weights, x and dL/dy (the fp64 network itself).
    masks: one bool [rows, width] per ReLU layer, the on / off pattern forced on it: h = z * mask, forward and backward."""
    assert order in ("accumulator", "rounded", "unrounded"), order
    exact = order == "unrounded"
    rnd = (lambda t: t.double()) if exact else (lambda t: t.half().double())
    keep = (lambda t: t) if exact else _Round.apply
    h0 = rnd(x.detach()).requires_grad_(True)
    h = h0
    ws = [rnd(l.weight.detach()).requires_grad_(True) for l in m.layers]
    bs = [None if l.bias is None else rnd(l.bias.detach()).requires_grad_(True) for l in m.layers]
    zs = []
    masks = None if masks is None else list(masks)
    for i, (l, W, b) in enumerate(zip(m.layers, ws, bs)):
        last = i + 1 == len(m.layers)
        z = torch.nn.functional.linear(h, W, b)
        if (round_pre and not last and l.activation is not None) or (order == "rounded" and last):
            z = _Round.apply(z)
        if _kind(l) == "relu":
            zs.append(z.detach())
            h = _activate(l, z) if masks is None else z * masks[len(zs) - 1].to(z.dtype)
        else:
            h = _activate(l, z)
        h = keep(h)
    assert masks is None or len(masks) == len(zs), "one mask per ReLU layer"
    h.backward(rnd(gy))
    return h.detach(), h0.grad, [w.grad for w in ws], [None if b is None else b.grad for b in bs], zs


def _ulp_of_half(h):
    """the spacing of half-precision numbers at h (2^-24 in the subnormal range and at 0)"""
    e = torch.frexp(h.abs())[1].double() - 1.0                    # floor(log2 |h|)
    e = torch.where(h == 0, torch.full_like(e, -14.0), e).clamp_min(-14.0)
    return torch.exp2(e - 10.0)


def flip_band(m, x, unrounded_operands=False):
    """-> one [rows, width] fp64 tensor per ReLU layer: dz, a bound on how far the kernel's pre-activation may sit from the contract's,
    computed from the contract alone.  Layer 0 (its input is x rounded to half, the same on both sides): the fp32 accumulation,
    (fan_in + 2) 2^-24 (|W| |h| + |b|).  Deeper layers add |W| dh, dh = dz of the layer before (every activation here is 1-Lipschitz)
    + one ulp of its half output: the kernel may round an activation the other way after fp32 accumulation.  All units of a row
    are taken to err at once and in the worst direction, so the band is wide (a tenth to a third of all rows has a unit inside it);
    it only limits which units assert_rows() may switch.  A unit is "near" when |z| <= dz.
    unrounded_operands: the band for an evaluation of the network on the fp32 parameters and x as they are (the half block's second
    order, models/blocks/mlp.py FusedMLPHalfFunction.backward) -- half rounding moves each of them by up to 2^-11 of itself, so every
    layer adds 2^-11 (|W| |h| + |b|) and x starts with dh = 2^-11 |x|."""
    rnd = lambda t: t.detach().half().double()
    with torch.no_grad():
        h = rnd(x)
        dh = 2.0 ** -11 * h.abs() if unrounded_operands else torch.zeros_like(h)
        out = []
        for l in m.layers:
            W = rnd(l.weight)
            b = None if l.bias is None else rnd(l.bias)
            z = torch.nn.functional.linear(h, W, b)
            mag = torch.nn.functional.linear(h.abs(), W.abs(), None if b is None else b.abs())
            dz = ((W.shape[1] + 2) * 2.0 ** -24 + (2.0 ** -11 if unrounded_operands else 0.0)) * mag + torch.nn.functional.linear(dh, W.abs())
            if _kind(l) == "relu":
                out.append(dz)
            h = rnd(_activate(l, z))
            dh = dz + _ulp_of_half(h)
    return out


def rows_in_band(zs, dzs):
    """bool [rows]: the row has a near unit in some ReLU layer"""
    near = torch.zeros(zs[0].shape[0], dtype=torch.bool, device=zs[0].device)
    for z, dz in zip(zs, dzs):
        near |= (z.abs() <= dz).any(1)
    return near


def near_units(zs, dzs, r):
    """the units of row r inside the band: [(relu layer, unit, z, dz)], smallest |z| first"""
    found = []
    for k, (z, dz) in enumerate(zip(zs, dzs)):
        zr, dr = z[r], dz[r]
        for u in torch.nonzero(zr.abs() <= dr).flatten().tolist():
            found.append((k, u, float(zr[u]), float(dr[u])))
    return sorted(found, key=lambda t: abs(t[2]))


def assert_rows(name, got, m, x, gy, tol, contract_kwargs=None, max_excused=0, contract=None):
    """every row of got (the kernel's dL/dx, [n, in]) against the contract: finite everywhere; a row is fine when max |got[r] - dx[r]|
    <= tol max |dx|; every other row must be excused by a proven kink -- of its near units (flip_band) the 8 with the smallest |z|, their
    subsets switched the other way (singles first), and for one of them half_contract on that row with the pattern forced matches got[r]
    within the same tol max |dx|.  A row without such a pattern fails; more than max_excused excused rows fail.
    contract: half_contract(m, x, gy, **contract_kwargs) where the caller has it already.
    -> [(row, ((relu layer, unit), ...))] of the excused rows"""
    kw = dict(contract_kwargs or {})
    n = got.shape[0]
    assert torch.isfinite(got).all(), f"{name}: {int((~torch.isfinite(got)).any(1).sum())} of {n} rows are not finite"
    _, dx, _, _, zs = contract if contract is not None else half_contract(m, x, gy, **kw)
    assert got.shape == dx.shape, f"{name}: shape {tuple(got.shape)} for {tuple(dx.shape)}"
    got = got.detach().double()
    bound = tol * (float(dx.abs().max()) or 1.0)
    err = (got - dx).abs().amax(1)
    off = torch.nonzero(~(err <= bound)).flatten().tolist()
    excused = []
    dzs = flip_band(m, x) if off and zs else []
    for r in off:
        where = f"{name}: row {r} of {n} (r % 32 = {r % 32}, r % 256 = {r % 256}) misses the contract by {float(err[r]) / bound:.2f} x the tolerance"
        assert zs, f"{where}; the network has no ReLU layer, so no row is excused"
        near = near_units(zs, dzs, r)
        units = near[:MAX_FLIP_UNITS]
        subsets = [s for k in range(1, len(units) + 1) for s in itertools.combinations(range(len(units)), k)]
        found = None
        if subsets:
            masks = [(z[r] > 0).unsqueeze(0).repeat(len(subsets), 1) for z in zs]
            for p, s in enumerate(subsets):
                for j in s:
                    k, u = units[j][:2]
                    masks[k][p, u] = ~masks[k][p, u]
            xr, gr = x[r:r + 1].detach().expand(len(subsets), -1), gy[r:r + 1].detach().expand(len(subsets), -1)
            dxp = half_contract(m, xr, gr, masks=masks, **kw)[1]
            ok = torch.nonzero((dxp - got[r]).abs().amax(1) <= bound).flatten().tolist()
            if ok:
                found = tuple(units[j][:2] for j in subsets[ok[0]])
        listing = ", ".join(f"layer {k} unit {u}: z = {z:.3e}, band {dz:.3e}" for k, u, z, dz in near) or "none"
        assert found is not None, f"{where} and no switched pattern of its near units explains it; near units: {listing}"
        excused.append((r, found))
        assert len(excused) <= max_excused, (f"{name}: more than {max_excused} of {n} rows need a kink to be excused "
                                             f"(rows {[e[0] for e in excused]}, {len(off)} rows off in all)")
    print(f"{name}: {len(excused)} of {n} rows excused by a proven kink (cap {max_excused}); {len(off)} off the plain tolerance")
    return excused


# ------------------------------------------------------------------------------------------------------------------------
# second order through the half block: rows against an fp64 twin of the module
# ------------------------------------------------------------------------------------------------------------------------
def double_twin(m, rounded=True):
    """the module in float64 on the layer-by-layer path: parameters rounded to half (rounded=False: as they are), everything else
    double.  Its x is the caller's: x.half().double() for the rounded twin"""
    import copy
    desc, m._desc = m._desc, None
    try:
        t = copy.deepcopy(m)
    finally:
        m._desc = desc
    t.dtype = torch.float64
    for l in t.layers:
        l.dtype = torch.float64                                   # no autocast in DenseLayer.forward
    t.double()
    if rounded:
        with torch.no_grad():
            for p in t.parameters():
                p.copy_(p.half().double())
    return t


def check_rows_against_twin(name, fused, unfused, twin, outside=None, unfused_twin=None, floor=2e-2, share=0.05):
    """row by row, max |a[r] - twin[r]| relative to max |twin|: the fused run is held to max(floor, 4 x the error of the USE_FUSED =
    False run of the same module) -- the project's yardstick, 4 x torch's own error -- in EVERY row (outside: in every row of that
    mask, and the rows outside the mask that miss it stay below `share` of all rows).  unfused_twin: the twin the USE_FUSED = False
    run is measured against, where that is another one than the fused run's.  -> (fused, unfused) errors"""
    twin = twin.double()
    unfused_twin = twin if unfused_twin is None else unfused_twin.double()
    scale = float(twin.abs().max()) or 1.0
    sel = torch.ones(twin.shape[0], dtype=torch.bool, device=twin.device) if outside is None else outside
    assert torch.isfinite(fused).all(), f"{name}: not finite"
    err = (fused.double() - twin).abs().amax(1) / scale
    err_t = (unfused.double() - unfused_twin).abs().amax(1) / scale
    e_f, e_t = float(err[sel].max()), float(err_t[sel].max())
    bound = max(floor, 4 * e_t)
    print(f"YARDSTICK {name}: worst row {e_f:.3e} of scale, USE_FUSED = False {e_t:.3e}, bound {bound:.3e}, "
          f"{int(sel.sum())} of {twin.shape[0]} rows judged one by one")
    worst = int(torch.where(sel, err, torch.zeros_like(err)).argmax())
    assert e_f <= bound, f"{name}: row {worst} (r % 32 = {worst % 32}, r % 256 = {worst % 256}) is off by {e_f:.3e} of scale, bound {bound:.3e}"
    rest = float(((err > bound) & ~sel).sum()) / twin.shape[0]
    assert rest < share, f"{name}: {rest:.3f} of the rows, all with a unit near its kink, differ"
    return e_f, e_t
