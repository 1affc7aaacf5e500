"""The NeuS render composite on the GPU (nr3d_neus_composite_fwd / _bwd through bindings._neus_composite and graphics.neus.neus_render),
rows and packs, with and without rgb / normals.

Yardstick (that of tests/test_neus_alpha_gpu.py): for every output and every gradient the error against the float64 evaluation of
the restated reference chain (tests/neus_render_ref.py), relative to the tensor's maximum, is at most max(1e-5, 4 x the error of
torch's fp32 chain on the same inputs and device).  Every check prints its ratio ("YARDSTICK ..."); profiles/neus_composite.json
keeps one run of them: 524 checks, the largest ratios 1.0 (vw), 3.87 (depth), 1.27 (rgb), 2.51 (normals), 2.31 (dL/dt), 1.0 (dL/drgb),
1.04 (dL/dnablas); mask reaches 160.6 at an error of 6.0e-08 and dL/dalpha 5.97 at 1.4e-06, both below the 1e-5 floor.

The pack inputs are asserted (float64) to hold no transmittance within a relative 1e-3 of early_stop_eps, so no sample's membership
depends on rounding and no element is left out of any comparison.  The tests set FUSED_NEUS_COMPOSITE themselves, so they cover the fused
route whatever its default is."""
import contextlib
import functools

import pytest
import torch

import neus_render_ref as ref

pytestmark = pytest.mark.gpu

FUSED_NODE = "NeusCompositeBackward"
ROW_SHAPES = [(1, 1), (3, 1), (5, 7), (4, 64), (3, 65), (2, 130), (257, 128), (2, 4200)]     # 4200: more than 64 chunks of 64 in the backward
PACK_COUNTS = [1, 5, 300]
# (with_rgb, with_nablas, normalize_depth, hit, with_g_vw)
COMBOS = [(True, True, True, True, True), (False, False, False, False, False), (True, False, True, False, True),
          (False, True, False, True, False)]


@contextlib.contextmanager
def _switch(on):
    from nr3d_lib_amd.graphics.neus import neus_render as nr
    saved = nr.FUSED_NEUS_COMPOSITE
    nr.FUSED_NEUS_COMPOSITE = on
    try:
        yield nr
    finally:
        nr.FUSED_NEUS_COMPOSITE = saved


def _check(name, got, ref64, ref32):
    scale = float(ref64.abs().max()) or 1.0
    err = float((got.double().cpu() - ref64.double().cpu()).abs().max()) / scale
    err32 = float((ref32.double().cpu() - ref64.double().cpu()).abs().max()) / scale
    print(f"YARDSTICK {name}: rel err {err:.3e} torch fp32 {err32:.3e} ratio {err / err32 if err32 else float('inf'):.2f}")
    assert got.shape == ref64.shape, f"{name}: shape {list(got.shape)}, expected {list(ref64.shape)}"
    assert torch.isfinite(got).all(), f"{name}: not finite"
    assert err <= max(1e-5, 4 * err32), f"{name}: rel err {err:.2e} (torch fp32 chain: {err32:.2e})"


@functools.lru_cache(maxsize=None)
def _inputs(layout, a, b, kind="random"):
    if layout == "rows":
        return ref.rows_inputs(a, b, kind=kind)
    return ref.pack_inputs(a, seed=b, gaps=layout == "packs")           # packs: b is the seed; "tiled": no gaps between the packs


@functools.lru_cache(maxsize=None)
def _bit_inputs(P):
    """packs for the bit-for-bit comparison of two kernels with the same arithmetic: no margin around early_stop_eps is needed (among
    2100 packs some transmittance always comes within 1e-3 of it)"""
    return ref.pack_inputs(P, margin=False)


@functools.lru_cache(maxsize=None)
def _refs(layout, a, b, kind, combo, normalized=False):
    """(float64 on the CPU, float32 on the GPU) evaluations of the chain, computed once per case"""
    rgb, nab, norm, hit, gvw = combo
    inp = _inputs(layout, a, b, kind)
    kw = dict(with_rgb=rgb, with_nablas=nab, hit=hit, normalize_depth=norm, normalized_normals=normalized, with_g_vw=gvw)
    return ref.evaluate(inp, torch.float64, "cpu", **kw), ref.evaluate(inp, torch.float32, "cuda:0", **kw)


def _run(inp, combo, dev, normalized=False, backward=True):
    """the fused route through the Python surface -> (dict of outputs and grads, the output tuple, the input leaves)"""
    rgb_on, nab_on, norm, hit_on, gvw = combo
    leaf = lambda a, on=True: torch.from_numpy(a).to(dev).requires_grad_(backward) if on else None     # noqa: E731
    alpha, t, rgb, nablas = leaf(inp["alpha"]), leaf(inp["t"]), leaf(inp["rgb"], rgb_on), leaf(inp["nablas"], nab_on)
    hit = torch.from_numpy(inp["rays_inds_hit"]).to(dev) if hit_on else None
    num_rays = inp["num_rays"] if hit_on else inp["P"]
    with _switch(True) as nr:
        if inp["layout"] == "rows":
            out = nr.ray_composite(alpha, t, rgb, nablas, hit, num_rays, normalize_depth=norm, normalized_normals=normalized)
        else:
            out = nr.packed_composite_normals(alpha, t, rgb, nablas, torch.from_numpy(inp["pack_infos"]).to(dev), hit, num_rays,
                                              normalize_depth=norm, normalized_normals=normalized)
    res = dict(zip(ref.OUTPUTS, (None if o is None else o.detach() for o in out)))
    if backward:
        assert FUSED_NODE in type(out[1].grad_fn).__name__ or (inp["layout"] == "packs" and not nab_on), type(out[1].grad_fn).__name__
        cot = ref.cotangents(inp)
        loss = 0
        for k, o in zip(ref.OUTPUTS, out):
            if o is not None and (k != "vw" or gvw):
                g = torch.from_numpy(cot[k]).to(dev)
                loss = loss + (o * (g if (hit_on or k == "vw") else g[:inp["P"]])).sum()
        wrt = [(k, x) for k, x in zip(ref.GRADS, (alpha, t, rgb, nablas)) if x is not None]
        for (k, x), g in zip(wrt, torch.autograd.grad(loss, [x for _, x in wrt], allow_unused=True)):
            res[k] = torch.zeros_like(x) if g is None else g
    return res, out, (alpha, t, rgb, nablas)


def _compare(tag, res, r64, r32):
    for k in ref.OUTPUTS + ref.GRADS:
        if r64.get(k) is not None:
            _check(f"{tag} {k}", res[k], r64[k], r32[k])
        else:
            assert res.get(k) is None, f"{tag}: unexpected {k}"


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "".join("01"[int(x)] for x in c))
def test_rows(dev, shape, combo):
    """every output and gradient of the rows layout inside the yardstick: with and without rgb / nablas, both normalize_depth values,
    with and without rays_inds_hit, with and without a gradient on vw"""
    res, _, _ = _run(_inputs("rows", *shape), combo, dev)
    _compare(f"rows {shape} {combo}", res, *_refs("rows", *shape, "random", combo))


@pytest.mark.parametrize("shape", [(5, 7), (3, 65), (6, 130), (3, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["opaque", "zero"])
def test_rows_opaque_and_zero(dev, shape, kind):
    """an exact alpha == 1 at the first, a middle and the last sample of a row (neus_ray_sdf_to_alpha's clamp reaches it): the gradient is
    finite and inside the yardstick at, before and after the opaque sample; and all-zero alpha"""
    inp = _inputs("rows", *shape, kind)
    res, _, _ = _run(inp, COMBOS[0], dev)
    r64, r32 = _refs("rows", *shape, kind, COMBOS[0])
    _compare(f"rows {kind} {shape}", res, r64, r32)
    if kind == "opaque":
        n = shape[1]
        col = torch.arange(n)[None, :]
        at = torch.from_numpy(inp["opaque_at"])[:, None]
        scale = float(r64["g_alpha"].abs().max())
        for name, sel in (("at", col == at), ("before", col < at), ("after", col > at)):
            if sel.any():
                got, want, want32 = (x.cpu()[sel] for x in (res["g_alpha"], r64["g_alpha"], r32["g_alpha"]))
                err, err32 = float((got.double() - want).abs().max()) / scale, float((want32.double() - want).abs().max()) / scale
                print(f"YARDSTICK rows opaque {shape} g_alpha {name}: rel err {err:.3e} torch fp32 {err32:.3e}")
                assert torch.isfinite(got).all() and err <= max(1e-5, 4 * err32), f"g_alpha {name} the opaque sample: {err:.2e}"
        assert (res["vw"].cpu()[col > at] == 0).all()              # nothing is seen behind an opaque sample


@pytest.mark.parametrize("P", PACK_COUNTS)
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "".join("01"[int(x)] for x in c))
@pytest.mark.parametrize("pack_scan", [1, 0])
def test_packs(dev, hip_option, P, combo, pack_scan):
    """every output and gradient of the packed layout (lengths 0, 1, 63, 64, 65, 200, gaps, shuffled rays_inds_hit) inside the yardstick,
    with the prefix-product kernels and with the serial ones"""
    hip_option("pack_scan", pack_scan)
    res, _, _ = _run(_inputs("packs", P, 0), combo, dev)
    _compare(f"packs {P} scan {pack_scan} {combo}", res, *_refs("packs", P, 0, "random", combo))


@pytest.mark.parametrize("P", PACK_COUNTS + [2100])                # 2100: the existing entry's lane-per-pack kernels (pack_scan 0)
@pytest.mark.parametrize("pack_scan", [1, 0])
def test_packs_without_nablas_equal_packed_composite(dev, hip_option, P, pack_scan):
    """with nablas NULL every output and gradient of the new entries equals the existing entries' bit for bit"""
    from nr3d_lib_amd.bindings import _neus_composite as nc, _pack_ops as po
    hip_option("pack_scan", pack_scan)
    inp = _bit_inputs(P)
    g = lambda a: torch.from_numpy(a).to(dev)           # noqa: E731
    alpha, t, rgb, pi, hit = g(inp["alpha"]), g(inp["t"]), g(inp["rgb"]), g(inp["pack_infos"]), g(inp["rays_inds_hit"])
    cot = {k: g(v) for k, v in ref.cotangents(inp).items()}
    for with_rgb in (True, False):
        c = rgb if with_rgb else None
        new = nc.neus_composite_forward(alpha, t, c, None, pi, hit, inp["num_rays"], 1e-4, 0.0, True, 0)
        old = po.packed_composite_forward(alpha, t, c, pi, hit, inp["num_rays"], 1e-4, 0.0, True)
        assert new[4] is None and (new[3] is None) == (not with_rgb)
        for name, a, b in zip(("vw", "mask", "depth", "rgb"), new, old):
            assert (a is None and b is None) or torch.equal(a, b), f"{name} differs (rgb {with_rgb})"
        g_rgb = cot["rgb"] if with_rgb else None
        new_g = nc.neus_composite_backward(alpha, t, c, None, pi, hit, 1e-4, 0.0, True, 0, new[0], new[1], new[2], cot["mask"],
                                           cot["depth"], g_rgb, None, cot["vw"])
        old_g = po.packed_composite_backward(alpha, old[0], t, c, pi, hit, 1e-4, 0.0, True, old[1], old[2], cot["mask"], cot["depth"],
                                             g_rgb, cot["vw"])
        assert new_g[3] is None
        for name, a, b in zip(("grad_alphas", "grad_t", "grad_rgb"), new_g, old_g):
            assert (a is None and b is None) or torch.equal(a, b), f"{name} differs (rgb {with_rgb})"


@pytest.mark.parametrize("case,pack_scan", [(("rows", 5, 7), 1), (("rows", 3, 65), 1), (("rows", 257, 128), 1), (("rows", 3, 1), 1),
                                            (("packs", 5, 0), 1), (("packs", 5, 0), 0), (("packs", 300, 0), 1), (("packs", 300, 0), 0)],
                         ids=lambda c: f"{c[0]}{c[1]}x{c[2]}" if isinstance(c, tuple) else f"scan{c}")
def test_normalized_normals(dev, hip_option, case, pack_scan):
    """normals_mode 1: the outputs inside the yardstick; the buffer's nablas afterwards = clamp(-1, 1) of the input bit for bit; zero
    nablas give zero normals, not NaN"""
    hip_option("pack_scan", pack_scan)
    inp = _inputs(*case)
    for combo in (COMBOS[0], COMBOS[3]):
        res, _, leaves = _run(inp, combo, dev, normalized=True, backward=False)
        r64, r32 = _refs(*case, "random", combo, True)
        for k in ref.OUTPUTS:
            if r64[k] is not None:
                _check(f"{case} unit normals {k}", res[k], r64[k], r32[k])
        before = torch.from_numpy(inp["nablas"])
        assert torch.equal(leaves[3].cpu(), before.clamp(-1, 1)), "nablas not clamped in place"
    zero = dict(inp, nablas=torch.zeros_like(before).numpy())
    res, _, _ = _run(zero, COMBOS[0], dev, normalized=True, backward=False)
    assert not res["normals"].any() and torch.isfinite(res["normals"]).all()


def test_fallback_for_normalized_normals_with_grad(dev):
    """the backward entry refuses normals_mode 1 with g_normals or grad_nablas; the Python layer takes the op chain instead of reaching it"""
    from nr3d_lib_amd.bindings import _neus_composite as nc
    inp = _inputs("rows", 5, 7)
    g = lambda a: torch.from_numpy(a).to(dev)           # noqa: E731
    alpha, t, rgb, nablas = g(inp["alpha"]), g(inp["t"]), g(inp["rgb"]), g(inp["nablas"])
    vw, mask, depth, _, normals = nc.neus_composite_forward(alpha, t, rgb, nablas, normals_mode=1)
    with pytest.raises(RuntimeError, match="forward only"):
        nc.neus_composite_backward(alpha, t, rgb, nablas, None, None, 0.0, 0.0, True, 1, vw, mask, depth, None, None, None,
                                   torch.ones_like(normals), None, need_nablas=False)
    with pytest.raises(RuntimeError, match="forward only"):
        nc.neus_composite_backward(alpha, t, rgb, nablas, None, None, 0.0, 0.0, True, 1, vw, mask, depth, torch.ones_like(mask), None, None,
                                   None, None, need_nablas=True)
    # rejected at the C boundary: unknown layout, unknown normals_mode, rows with pack_infos, n == 0 with P > 0
    from nr3d_lib_amd import _hip as H
    pi = torch.zeros(5, 2, dtype=torch.int64, device=dev)
    for layout, S, n, pack_infos, mode in ((2, 35, 7, None, 0), (0, 35, 7, None, 2), (0, 35, 7, H.ptr(pi), 0), (0, 0, 0, None, 0)):
        rc = H.lib().nr3d_neus_composite_fwd(layout, 5, S, n, H.ptr(alpha), H.ptr(t), None, None, pack_infos, None, 0.0, 0.0, 1, mode,
                                             H.ptr(vw), H.ptr(mask), H.ptr(depth), None, None, None)
        assert rc != 0, (layout, S, n, mode)
    # the Python layer: a gradient is wanted and the normals are the normalised ones -> the chain, which autograd differentiates
    with _switch(True) as nr:
        a = alpha.clone().requires_grad_(True)
        nab = g(inp["nablas"])
        out = nr.ray_composite(a, t, rgb, nab, normalized_normals=True)
        assert FUSED_NODE not in type(out[4].grad_fn).__name__
        (ga,) = torch.autograd.grad(out[4].sum(), [a])
        assert torch.isfinite(ga).all() and torch.equal(nab.cpu(), torch.from_numpy(inp["nablas"]).clamp(-1, 1))
        with torch.no_grad():
            out = nr.ray_composite(a, t, rgb, g(inp["nablas"]), normalized_normals=True)           # no gradient recorded: the kernel
        assert out[4].grad_fn is None


@pytest.mark.parametrize("case", [("rows", 257, 128), ("rows", 2, 4200), ("packs", 300, 0)], ids=lambda c: f"{c[0]}{c[1]}x{c[2]}")
def test_deterministic(dev, case):
    """two runs give identical bytes, outputs and gradients"""
    inp = _inputs(*case)
    a, _, _ = _run(inp, COMBOS[0], dev)
    b, _, _ = _run(inp, COMBOS[0], dev)
    for k in ref.OUTPUTS + ref.GRADS:
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs"


def _buffer(inp, dev, grad):
    g = lambda a: torch.from_numpy(a).to(dev)           # noqa: E731
    buf = dict(type="batched" if inp["layout"] == "rows" else "packed", opacity_alpha=g(inp["alpha"]).requires_grad_(grad), t=g(inp["t"]),
               rgb=g(inp["rgb"]).requires_grad_(grad), nablas=g(inp["nablas"]).requires_grad_(grad), rays_inds_hit=g(inp["rays_inds_hit"]))
    if inp["pack_infos"] is not None:
        buf["pack_infos_hit"] = g(inp["pack_infos"])
        if int(inp["pack_infos"][:, 1].sum()) == inp["alpha"].shape[0]:
            from nr3d_lib_amd import _hip
            _hip.mark_ordered(buf["pack_infos_hit"], total=inp["alpha"].shape[0])
    return buf


@pytest.mark.parametrize("case", [("rows", 5, 7), ("rows", 257, 128), ("packs", 300, 0), ("tiled", 300, 0)],
                         ids=lambda c: f"{c[0]}{c[1]}x{c[2]}")
@pytest.mark.parametrize("training", [True, False])
def test_switch(dev, case, training):
    """composite_volume_buffer on GPU buffers gives the same result, inside the yardstick, with FUSED_NEUS_COMPOSITE on and off; the
    autograd graph holds the fused node only with the switch on.  "packs": with gaps (the chain's sums are index ops under a gradient);
    "tiled": the packs tile the buffer and are marked so, as a query's pack_infos_hit (the chain's sums are the library's pack ops)"""
    inp = _inputs(*case)
    r64, r32 = _refs(*case, "random", COMBOS[0], not training)
    for on in (True, False):
        buf = _buffer(inp, dev, grad=training)
        with _switch(on) as nr:
            out = nr.composite_volume_buffer(buf, inp["num_rays"], training=training)
        _check(f"switch {on} {case} vw", buf["vw"].detach(), r64["vw"], r32["vw"])
        for k, name in (("mask", "mask_volume"), ("depth", "depth_volume"), ("rgb", "rgb_volume"), ("normals", "normals_volume")):
            _check(f"switch {on} {case} {name}", out[name].detach(), r64[k], r32[k])
        if training:
            assert (FUSED_NODE in type(out["normals_volume"].grad_fn).__name__) == on
            cot = ref.cotangents(inp)
            loss = sum((out[name] * torch.from_numpy(cot[k]).to(dev)).sum() for k, name in
                       (("mask", "mask_volume"), ("depth", "depth_volume"), ("rgb", "rgb_volume"), ("normals", "normals_volume")))
            loss = loss + (buf["vw"] * torch.from_numpy(cot["vw"]).to(dev)).sum()
            grads = torch.autograd.grad(loss, [buf["opacity_alpha"], buf["rgb"], buf["nablas"]])
            for k, got in zip(("g_alpha", "g_rgb", "g_nablas"), grads):
                _check(f"switch {on} {case} {k}", got, r64[k], r32[k])
        else:
            assert torch.equal(buf["nablas"].cpu(), torch.from_numpy(inp["nablas"]).clamp(-1, 1))


def test_volume_buffer_empty_on_gpu(dev):
    with _switch(True) as nr:
        out = nr.composite_volume_buffer(dict(type="empty"), 9, device=dev)
    assert all(v.is_cuda and not v.any() for v in out.values()) and out["normals_volume"].shape == (9, 3)
