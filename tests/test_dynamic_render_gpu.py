"""``composite_static_dynamic`` (graphics/nerf/nerf_dynamic_render.py) on packed buffers on the GPU, forward and backward, against a
float64 restatement of the reference's packed branch (nr3d_lib/models/fields_dynamic/nerf/emernerf.py:806-811, :883-938).

The restatement is numpy for the forward (``restate``); the same chain in torch float64 on the CPU supplies the gradients, after its
forward is held to the numpy one at 1e-12.  Yardstick, that of tests/test_neus_render_gpu.py:49 for the same quantities on packs (mask,
depth, rgb, normals and their gradients): the error against the float64 chain, relative to the tensor's maximum, is at most
max(1e-5, 4 x the error of the float32 torch-op chain on the same inputs and device).  The inputs are asserted (float64) to hold no
transmittance within a relative 1e-3 of early_stop_eps (as tests/neus_render_ref.py::pack_inputs does), so no sample's membership
depends on rounding."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-4
LENGTHS = (0, 1, 2, 63, 64, 65, 130)         # both sides of a wave, two waves and a bit
FLOWS = ("flow_fwd", "flow_bwd")
LEAVES = ("sigma_static", "sigma_dynamic", "t", "rgb_static", "rgb_dynamic", "nablas_static", "nablas_dynamic") + FLOWS
SIDES = ("static", "dynamic")


@functools.lru_cache(maxsize=None)
def _inputs(reps, seed=0):
    """the first seed from `seed` on whose packs keep every transmittance a relative 1e-3 away from early_stop_eps"""
    for s in range(seed, seed + 64):
        try:
            return _draw(reps, s)
        except AssertionError:
            continue
    raise RuntimeError("no seed with a margin around early_stop_eps")


def _draw(reps, seed):
    rng = np.random.default_rng(seed)
    lens = np.array(LENGTHS * reps, dtype=np.int64)
    rng.shuffle(lens)
    first = np.cumsum(lens) - lens
    S, P = int(lens.sum()), len(lens)
    num_rays = P + 3
    inp = dict(pack_infos=np.stack([first, lens], 1), rays_inds_hit=rng.permutation(num_rays)[:P].astype(np.int64), num_rays=num_rays, S=S,
               deltas=rng.uniform(0.01, 0.05, S).astype(np.float32), t=rng.uniform(0.5, 6.0, S).astype(np.float32))
    for side, peak in zip(SIDES, (6.0, 25.0)):
        inp["sigma_" + side] = (rng.random(S) ** 2 * np.repeat(rng.choice([0.2, 1.0], P), lens) * peak).astype(np.float32)
        inp["rgb_" + side] = rng.random((S, 3)).astype(np.float32)
        inp["nablas_" + side] = rng.standard_normal((S, 3)).astype(np.float32)
        alpha = 1.0 - np.exp(-inp["sigma_" + side].astype(np.float64) * inp["deltas"])
        for f, n in zip(first, lens):
            T = np.cumprod(np.concatenate([[1.0], 1.0 - alpha[f:f + n]]))
            assert (np.abs(T - EPS) > 1e-3 * EPS).all(), f"{side}: a transmittance within 1e-3 of early_stop_eps (seed {seed})"
    for k in FLOWS:
        inp[k] = rng.standard_normal((S, 3)).astype(np.float32)
    inp["cot"] = {k: rng.standard_normal((num_rays,) + ((3,) if dim3 else ())).astype(np.float32)
                  for k, dim3 in [(f"{q}_{s}", q in ("rgb", "normals")) for q in ("mask", "depth", "rgb", "normals") for s in SIDES]
                  + [(k, True) for k in FLOWS]}
    return inp


def restate(inp, normalize_depth, training=True):
    """emernerf.py:806-811 and :908-938 in numpy float64, pack by pack"""
    a = {k: np.asarray(v, np.float64) for k, v in inp.items() if isinstance(v, np.ndarray) and v.dtype == np.float32}
    n = inp["num_rays"]
    out = {f"{q}_{s}": np.zeros((n,) + ((3,) if q in ("rgb", "normals") else ())) for q in ("mask", "depth", "rgb", "normals") for s in SIDES}
    out.update({k: np.zeros((n, 3)) for k in FLOWS})
    for (first, cnt), ray in zip(inp["pack_infos"], inp["rays_inds_hit"]):
        sl = slice(first, first + cnt)
        for side in SIDES:
            alpha = 1.0 - np.exp(-a["sigma_" + side][sl] * a["deltas"][sl])             # tau_to_alpha(sigma * deltas)
            T = np.cumprod(np.concatenate([[1.0], 1.0 - alpha]))[:-1]
            vw = np.where(T < EPS, 0.0, alpha * T)                                      # packed_alpha_to_vw: early stop at 1e-4
            out["mask_" + side][ray] = s = vw.sum()
            out["depth_" + side][ray] = ((vw / (s + 1e-10)) * a["t"][sl]).sum() if normalize_depth else (vw * a["t"][sl]).sum()
            out["rgb_" + side][ray] = (vw[:, None] * a["rgb_" + side][sl]).sum(0)
            nab = a["nablas_" + side][sl]
            if not training:
                nab = np.clip(nab, -1, 1)
                nab = nab / np.maximum(np.linalg.norm(nab, axis=-1, keepdims=True), 1e-12)
            out["normals_" + side][ray] = (vw[:, None] * nab).sum(0)
            if side == "dynamic":                                                       # flows: rendered with vw_dynamic
                for k in FLOWS:
                    out[k][ray] = (vw[:, None] * a[k][sl]).sum(0)
    return out


def torch_chain(inp, dtype, device, normalize_depth, training=True, backward=True):
    """the same chain in torch ops (index ops per pack) -> (outputs, gradients with respect to LEAVES under the cotangents)"""
    from nr3d_lib_amd.graphics.neus.neus_render import _packed_alpha_to_vw_torch, _packed_div_torch, _packed_sum_torch, _scatter
    leaf = {k: torch.from_numpy(inp[k]).to(device=device, dtype=dtype).requires_grad_(backward) for k in LEAVES}
    deltas = torch.from_numpy(inp["deltas"]).to(device=device, dtype=dtype)
    pi, hit, n = torch.from_numpy(inp["pack_infos"]).to(device), torch.from_numpy(inp["rays_inds_hit"]).to(device), inp["num_rays"]
    out = {}
    for side in SIDES:
        alpha = 1 - torch.exp(-leaf["sigma_" + side] * deltas)
        vw = _packed_alpha_to_vw_torch(alpha, pi, EPS, 0.0)
        s = _packed_sum_torch(vw, pi)
        w = _packed_div_torch(vw, s + 1e-10, pi) if normalize_depth else vw
        nab = leaf["nablas_" + side]
        if not training:
            nab = torch.nn.functional.normalize(nab.clamp(-1, 1), dim=-1)
        out["mask_" + side], out["depth_" + side] = _scatter(s, hit, n), _scatter(_packed_sum_torch(w * leaf["t"], pi), hit, n)
        out["rgb_" + side] = _scatter(_packed_sum_torch(vw[:, None] * leaf["rgb_" + side], pi), hit, n)
        out["normals_" + side] = _scatter(_packed_sum_torch(vw[:, None] * nab, pi), hit, n)
        if side == "dynamic":
            for k in FLOWS:
                out[k] = _scatter(_packed_sum_torch(vw[:, None] * leaf[k], pi), hit, n)
    return out, (_grads(inp, out, leaf, device, dtype) if backward else None)


def _grads(inp, out, leaf, device, dtype):
    loss = sum((out[k] * torch.from_numpy(c).to(device=device, dtype=dtype)).sum() for k, c in inp["cot"].items())
    gs = torch.autograd.grad(loss, [leaf[k] for k in LEAVES], allow_unused=True)
    return {k: torch.zeros_like(leaf[k]) if g is None else g for k, g in zip(LEAVES, gs)}


def _check(name, got, ref64, ref32):
    scale = float(ref64.abs().max()) or 1.0
    err = float((got.double().cpu() - ref64.double().cpu()).abs().max()) / scale
    err32 = float((ref32.double().cpu() - ref64.double().cpu()).abs().max()) / scale
    print(f"YARDSTICK {name}: rel err {err:.3e} torch fp32 {err32:.3e} ratio {err / err32 if err32 else float('inf'):.2f}")
    assert got.shape == ref64.shape, f"{name}: shape {list(got.shape)}, expected {list(ref64.shape)}"
    assert torch.isfinite(got).all(), f"{name}: not finite"
    assert err <= max(1e-5, 4 * err32), f"{name}: rel err {err:.2e} (torch fp32 chain: {err32:.2e})"      # test_neus_render_gpu.py:49


def _buffer(inp, dev, backward, tiles=True):
    from nr3d_lib_amd import _hip as H
    leaf = {k: torch.from_numpy(inp[k]).to(dev).requires_grad_(backward) for k in LEAVES}
    pi = torch.from_numpy(inp["pack_infos"]).to(dev)
    if tiles:
        H.mark_ordered(pi, total=inp["S"])       # what a ray query's pack_infos_hit carry
    vb = dict(type="packed", pack_infos_hit=pi, rays_inds_hit=torch.from_numpy(inp["rays_inds_hit"]).to(dev),
              deltas=torch.from_numpy(inp["deltas"]).to(dev), **leaf)
    return vb, leaf


@pytest.mark.parametrize("tiles", [True, False], ids=["marked-tiling", "unmarked"])
@pytest.mark.parametrize("normalize_depth", [True, False], ids=["normalized-depth", "raw-depth"])
@pytest.mark.parametrize("reps", [1, 40], ids=["7-packs", "280-packs"])
def test_static_dynamic_packs_forward_and_backward(dev, reps, normalize_depth, tiles):
    from nr3d_lib_amd.graphics.nerf.nerf_dynamic_render import composite_static_dynamic
    inp = _inputs(reps)
    assert sorted(set(inp["pack_infos"][:, 1].tolist())) == sorted(LENGTHS)
    want_np = restate(inp, normalize_depth)
    r64, g64 = torch_chain(inp, torch.float64, "cpu", normalize_depth)
    for k, v in want_np.items():        # the torch float64 chain IS the numpy restatement
        assert np.abs(r64[k].detach().numpy() - v).max() <= 1e-12 * max(1.0, np.abs(v).max()), k
    r32, g32 = torch_chain(inp, torch.float32, dev, normalize_depth)
    vb, leaf = _buffer(inp, dev, True, tiles)
    out = composite_static_dynamic(vb, inp["num_rays"], with_rgb=True, with_normal=True, with_flow=True, training=True,
                                   depth_use_normalized_vw=normalize_depth)
    assert set(out) == set(want_np)
    assert "opacity_alpha_static" in vb and "opacity_alpha_dynamic" in vb and "vw_static" in vb and "vw_dynamic" in vb
    for k in want_np:
        _check(f"{reps} {k}", out[k].detach(), r64[k].detach(), r32[k].detach())
    got = _grads(inp, out, leaf, dev, torch.float32)
    for k in LEAVES:
        _check(f"{reps} dL/d{k}", got[k], g64[k], g32[k])
    # rays outside rays_inds_hit, and the rays of empty packs, stay zero
    quiet = np.setdiff1d(np.arange(inp["num_rays"]), inp["rays_inds_hit"][inp["pack_infos"][:, 1] > 0])
    assert quiet.size >= 3 and all(float(out[k].detach()[torch.from_numpy(quiet).to(dev)].abs().max()) == 0.0 for k in out)


def test_evaluation_normals_options_and_empty(dev):
    from nr3d_lib_amd.graphics.nerf.nerf_dynamic_render import composite_static_dynamic
    inp = _inputs(3, seed=2)
    r64, _ = torch_chain(inp, torch.float64, "cpu", True, training=False, backward=False)
    want_np = restate(inp, True, training=False)
    assert np.abs(r64["normals_dynamic"].numpy() - want_np["normals_dynamic"]).max() <= 1e-12
    r32, _ = torch_chain(inp, torch.float32, dev, True, training=False, backward=False)
    vb, _ = _buffer(inp, dev, False)
    with torch.no_grad():
        out = composite_static_dynamic(vb, inp["num_rays"], with_rgb=True, with_normal=True, with_flow=True, training=False)
    for k in ("normals_static", "normals_dynamic", "mask_static", "depth_dynamic", "flow_fwd"):
        _check(f"eval {k}", out[k], r64[k], r32[k])
    assert float(vb["nablas_static"].abs().max()) <= 1.0          # clamped in place, as the reference's clamp_
    # options: no rgb / normals / flows asked for, none returned; given alphas are used as they are
    vb, _ = _buffer(inp, dev, False)
    vb["opacity_alpha_static"] = torch.zeros(inp["S"], device=dev)
    with torch.no_grad():
        out = composite_static_dynamic(vb, inp["num_rays"], with_rgb=False, with_normal=False, with_flow=False)
    assert sorted(out) == ["depth_dynamic", "depth_static", "mask_dynamic", "mask_static"]
    assert float(out["mask_static"].abs().max()) == 0.0 and float(out["mask_dynamic"].max()) > 0.1
    # a buffer without nablas_static: its normals stay zero; the flows the buffer lacks are left out, fwd / bwd always present
    vb, _ = _buffer(inp, dev, False)
    del vb["nablas_static"], vb["flow_bwd"]
    with torch.no_grad():
        out = composite_static_dynamic(vb, inp["num_rays"], with_rgb=True, with_normal=True, with_flow=True)
    assert float(out["normals_static"].abs().max()) == 0.0 and float(out["normals_dynamic"].abs().max()) > 0
    assert float(out["flow_bwd"].abs().max()) == 0.0 and float(out["flow_fwd"].abs().max()) > 0 and "flow_fwd_pred_bwd" not in out
    empty = composite_static_dynamic(dict(type="empty", rays_inds_hit=[]), 5, with_rgb=True, with_normal=True, with_flow=True, device=dev)
    assert sorted(empty) == sorted(["mask_static", "mask_dynamic", "depth_static", "depth_dynamic", "rgb_static", "rgb_dynamic",
                                    "normals_static", "normals_dynamic", "flow_fwd", "flow_bwd"])
    assert all(v.shape[0] == 5 and float(v.abs().sum()) == 0.0 and v.device.type == "cuda" for v in empty.values())
