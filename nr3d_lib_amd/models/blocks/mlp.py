"""MLP blocks -- counterpart of ``MLP`` / ``FCBlock`` (nr3d_lib/models/blocks/mlp.py:27-127): D hidden ``DenseLayer``s of
width(s) W and an output layer, optional skip connections.  Same constructor, parameter names (``layers.{i}.weight`` /
``.bias``: checkpoints carry over) and forward signature.

Where the reference runs one GEMM + one activation kernel per layer (or hands the network to tiny-cuda-nn), this module
runs the whole network in ONE kernel on the fp32 MFMA (csrc/mlp.hip) -- or, for ``dtype=torch.half`` (the reference's autocast
layers / its tcnn FullyFusedMLP), on the f16 MFMA (csrc/mlp_half.hip) -- whenever it can: on a GPU, ReLU / no
activations or softplus hidden layers with beta >= ``FUSED_SOFTPLUS_MIN_BETA`` (the reference's SDF decoders:
``{'type': 'softplus', 'beta': 100.}``), a ReLU, sigmoid (the reference's radiance decoders: ``output_activation='sigmoid'``) or no
output activation, no skips / weight norm / equal_lr, every width <= 128.  Forward: activations stay in registers.  Backward
(hidden width <= 64): the forward is recomputed from x inside the backward kernel, so autograd keeps x and nothing else.
Everything else takes the layer-by-layer torch path below, with identical semantics.

Second order (``create_graph=True``: nablas = d sdf / dx and an eikonal loss on them, LoTDSDF.forward_sdf_nablas): the first
backward is the same fused kernel, wrapped as ``FusedMLPBackwardFunction``, and the loss's backward through the nablas runs the fused
double backward (csrc/mlp.hip k_mlp_bwd2, ``FUSED_SECOND_ORDER``) for both the fp32 and the half block (the half block's second order
is evaluated in fp32 from the fp32 parameters, as its torch route does).  The double backward gives x no gradient (ReLU / linear
networks: it is zero), so ``x.grad`` stays None when the eikonal term is x's only consumer.  A softplus network is not piecewise
linear -- the eikonal term does give x and the hidden biases a gradient, and there is a sigma'' chain -- so it has a double backward
kernel of its own (csrc/mlp_softplus2.hip k_mlp_bwd2_sp, ``desc.softplus_second_order_fusable``; ``desc.second_order_fusable`` stays False for
it), taken when ``FUSED_SOFTPLUS_SECOND_ORDER`` is on: the nablas are then the fused first backward's dL/dx bit for bit.  With the switch
off its create_graph backward differentiates the layer-by-layer torch evaluation of the same network -- which is also the route of a
block with a sigmoid output, whatever its hidden layers: no double backward kernel takes it (both ``..._second_order_fusable`` are False).

``LipshitzMLP`` (nr3d_lib/models/blocks/mlp.py:168-249) is the same network on weights normalised to a learnable bound per layer: the
normalisation of all layers is one launch each way (csrc/mlp_lipschitz.hip, ``LipschitzNormalizeFunction``, ``FUSED_LIPSHITZ``), and the
normalised weights take the routes above in place of the raw ones."""
from typing import List, Union

import torch
import torch.nn as nn

from nr3d_lib_amd.models.embedders import get_embedder
from nr3d_lib_amd.models.layers import DenseLayer, get_nonlinearity
from nr3d_lib_amd.profile import profile

__all__ = ['MLP', 'FCBlock', 'MLPNet', 'LipshitzMLP', 'FusedMLPFunction', 'FusedMLPHalfFunction', 'FusedMLPBackwardFunction',
           'LipschitzNormalizeFunction']

USE_FUSED = True                       # False: always the layer-by-layer path (A/B measurements, debugging)
# False: a create_graph backward of a fused block differentiates the layer-by-layer torch evaluation (the route before the fused double
# backward; A/B measurements, tests)
FUSED_SECOND_ORDER = True
# True: softplus networks take the fused route above too, through their own double backward kernel (k_mlp_bwd2_sp).  Needs
# FUSED_SECOND_ORDER.  False: their create_graph backward differentiates the torch evaluation.  DESIGN 7b has the measurements behind the default.
FUSED_SOFTPLUS_SECOND_ORDER = True
# True: a LipshitzMLP on the GPU normalises the weights of all its layers in one launch (LipschitzNormalizeFunction) and hands them to the
# routes of MLP, the fused decoder included.  False: the reference's torch chain, layer by layer.  README has the measurements behind the default.
FUSED_LIPSHITZ = True


def _fused_second_order(desc):
    """does a create_graph backward of this network return the fused first backward (FusedMLPBackwardFunction)?"""
    return FUSED_SECOND_ORDER and (desc.second_order_fusable or (FUSED_SOFTPLUS_SECOND_ORDER and desc.softplus_second_order_fusable))
# nn.Softplus hidden layers run on the fused kernels from this beta up (threshold 20, one beta for all hidden layers); below it they
# keep the layer-by-layer path.  The line is the one at which get_nonlinearity (models/layers.py; the reference's layers.py:212) already
# treats softplus as ReLU-like; every softplus of the reference has beta = 100, and the default nn.Softplus (beta = 1) stays on torch.
FUSED_SOFTPLUS_MIN_BETA = 5.0
# Reuse of the MFMA-ordered weight copy between calls.  OFF by default: packing is one ~3 us kernel, and the only cheap
# change detector -- the parameters' (data_ptr, _version) -- does not see in-place edits made through `.data`
# (EMA swaps `p.data.copy_(shadow)`, weight clipping, `.data.normal_()` re-initialisation), after which a cached copy
# would silently be stale.  Opt in for inference loops over frozen weights; `MLP.invalidate_packed()` (also called by
# `train()` / `eval()` / `load_state_dict()`) drops the copy explicitly.
CACHE_PACKED = False


def _torch_activation(h, desc, hidden):
    """the activation behind a hidden / the output layer of ``desc`` in torch (the differentiable re-evaluations below)"""
    from nr3d_lib_amd.bindings import _mlp
    act = desc.hidden_activation if hidden else desc.output_activation
    if act == _mlp.ACT_RELU:
        return torch.relu(h)
    if act == _mlp.ACT_SOFTPLUS:
        return torch.nn.functional.softplus(h, desc.beta, 20.0)
    if act == _mlp.ACT_SIGMOID:
        return torch.sigmoid(h)
    return h


class FusedMLPFunction(torch.autograd.Function):
    """y = MLP(x) through nr3d_mlp_forward; backward through nr3d_mlp_backward (recomputes the forward).
    args: desc, need (bool: a gradient may be asked for -> also pack the transposed layers), x, W_0, b_0 | None, W_1, ...

    Higher order (``create_graph=True``, e.g. the eikonal term on nablas = d sdf / dx): backward() then runs with grad
    mode on and returns the outputs of ``FusedMLPBackwardFunction`` -- the same fused kernel, whose own backward is the fused
    double backward (or, with ``FUSED_SECOND_ORDER = False`` / outside its range -- softplus hidden layers with
    ``FUSED_SOFTPLUS_SECOND_ORDER = False`` among it --, the gradients
    of a layer-by-layer PyTorch evaluation of the same network on the saved inputs, which autograd can differentiate again).  First-order training never
    takes that branch."""

    @staticmethod
    def forward(ctx, desc, need, x, *params):
        from nr3d_lib_amd.bindings import _mlp
        ws, bs = list(params[0::2]), list(params[1::2])
        # opt-in (CACHE_PACKED): the packed copy is keyed on the parameters alone; a copy packed with the transposed
        # layers (with_backward) also serves forward-only calls, a forward-only copy is upgraded when `need` first is True
        packed = None
        if CACHE_PACKED:
            key = tuple((p.data_ptr(), p._version) for p in params if p is not None)
            cached = getattr(desc, '_packed_cache', None)
            if cached is not None and cached[0] == key and (cached[2] or not need):
                packed = cached[1]
        if packed is None:
            packed = _mlp.pack(desc, ws, bs, with_backward=need)
            if CACHE_PACKED:
                desc._packed_cache = (key, packed, bool(need))
        if need:
            ctx.save_for_backward(x, packed, *[p for p in params if p is not None])
            ctx.desc, ctx.has_bias = desc, [b is not None for b in bs]
        return _mlp.forward(desc, x, packed)

    @staticmethod
    def backward(ctx, dL_dy):
        from nr3d_lib_amd.bindings import _mlp
        x, packed, *flat = ctx.saved_tensors
        n_layers = len(ctx.has_bias)
        if torch.is_grad_enabled():
            if _fused_second_order(ctx.desc):
                return (None, None, *FusedMLPBackwardFunction.apply(ctx.desc, packed, tuple(ctx.has_bias), tuple(ctx.needs_input_grad[2:]),
                                                                    x, dL_dy.float(), *flat))
            return (None, None, *FusedMLPFunction._differentiable_backward(ctx, x, flat, dL_dy))
        dx, dWs, dbs = _mlp.backward(ctx.desc, x, dL_dy.float(), packed, need_dx=ctx.needs_input_grad[2], has_bias=ctx.has_bias)
        grads = []
        for i in range(n_layers):
            grads += [dWs[i] if ctx.needs_input_grad[3 + 2 * i] else None,
                      dbs[i] if (dbs[i] is not None and ctx.needs_input_grad[4 + 2 * i]) else None]
        return (None, None, dx, *grads)

    @staticmethod
    def _differentiable_backward(ctx, x, flat, dL_dy):
        """(dL/dx, dL/dW_0, dL/db_0, ...) as differentiable functions of x, the parameters and dL/dy"""
        from nr3d_lib_amd.bindings import _mlp
        it = iter(flat)
        ws, bs = [], []
        for hb in ctx.has_bias:
            ws.append(next(it))
            bs.append(next(it) if hb else None)
        with torch.enable_grad():
            h = x if x.requires_grad else x.detach().requires_grad_(ctx.needs_input_grad[2])
            x_in = h
            for l, (W, b) in enumerate(zip(ws, bs)):
                h = torch.nn.functional.linear(h, W, b)
                h = _torch_activation(h, ctx.desc, l + 1 < len(ws))
            wanted, slots = [], []
            if ctx.needs_input_grad[2]:
                wanted.append(x_in); slots.append(0)
            for l, (W, b) in enumerate(zip(ws, bs)):
                if ctx.needs_input_grad[3 + 2 * l]:
                    wanted.append(W); slots.append(1 + 2 * l)
                if b is not None and ctx.needs_input_grad[4 + 2 * l]:
                    wanted.append(b); slots.append(2 + 2 * l)
            got = torch.autograd.grad(h, wanted, dL_dy, create_graph=True, allow_unused=True) if wanted else ()
        out = [None] * (1 + 2 * len(ws))
        for s_, g in zip(slots, got):
            out[s_] = g
        return out


class FusedMLPHalfFunction(torch.autograd.Function):
    """y = MLP(x) in half precision through nr3d_mlp_half_forward / _backward (csrc/mlp_half.hip, f16 MFMA): what the
    reference gets from tiny-cuda-nn's FullyFusedMLP (``use_tcnn_backend``, nr3d_lib/models/tcnn_adapter.py:37-51,74-146) and,
    numerically, what its ``DenseLayer(dtype=half)`` chain computes under autocast (half operands, fp32 accumulation, half
    activations between the layers).  The parameters stay fp32 (as in the reference's DenseLayer): they are rounded to half when
    packed, their gradients come back as the fp32 sums the kernel accumulated.  x may be float or half; y is half; dL/dx has
    x's dtype.  args: desc, need, x, W_0, b_0 | None, W_1, ...  Higher order: as FusedMLPFunction."""

    @staticmethod
    def forward(ctx, desc, need, x, *params):
        from nr3d_lib_amd.bindings import _mlp
        ws, bs = list(params[0::2]), list(params[1::2])
        packed = _mlp.pack_half(desc, ws, bs, with_backward=need)
        xh = x if x.dtype == torch.float16 else x.half()
        if need:
            # the CALLER's x is saved, not its rounded copy: the create_graph branch of the backward differentiates through it (a
            # detached x.half() was a fresh leaf: higher-order terms w.r.t. x never reached the caller's tensor -- round-4 advisor)
            ctx.save_for_backward(x, packed, *[p for p in params if p is not None])
            ctx.desc, ctx.has_bias, ctx.x_dtype = desc, [b is not None for b in bs], x.dtype
        return _mlp.forward_half(desc, xh, packed)

    @staticmethod
    def backward(ctx, dL_dy):
        from nr3d_lib_amd.bindings import _mlp
        x, packed, *flat = ctx.saved_tensors
        n_layers = len(ctx.has_bias)
        if torch.is_grad_enabled():
            # differentiable form: ONE dtype for x, the (fp32) parameters and dL/dy -- F.linear(half, float) raises outside
            # autocast; the casts are differentiable, so the graph reaches the caller's x whatever its dtype.  Fused: the same fp32
            # network through the fp32 kernels (the fp32 parameters packed here), so the semantics do not change
            if _fused_second_order(ctx.desc):
                ws, bs = FusedMLPBackwardFunction._params(ctx.has_bias, flat)
                packed32 = _mlp.pack(ctx.desc, ws, bs, with_backward=True)
                out = list(FusedMLPBackwardFunction.apply(ctx.desc, packed32, tuple(ctx.has_bias), tuple(ctx.needs_input_grad[2:]),
                                                          x.float(), dL_dy.float(), *flat))
            else:
                out = FusedMLPFunction._differentiable_backward(ctx, x.float(), flat, dL_dy.float())
            out[0] = None if out[0] is None else out[0].to(ctx.x_dtype)
            return (None, None, *out)
        xh = x if x.dtype == torch.float16 else x.half()
        dx, dWs, dbs = _mlp.backward_half(ctx.desc, xh, dL_dy.half(), packed, need_dx=ctx.needs_input_grad[2], has_bias=ctx.has_bias)
        grads = []
        for i in range(n_layers):
            grads += [dWs[i] if ctx.needs_input_grad[3 + 2 * i] else None,
                      dbs[i] if (dbs[i] is not None and ctx.needs_input_grad[4 + 2 * i]) else None]
        return (None, None, None if dx is None else dx.to(ctx.x_dtype), *grads)


class FusedMLPBackwardFunction(torch.autograd.Function):
    """The fused first backward as a differentiable op: (dL/dx, dL/dW_0, dL/db_0, ...) = nr3d_mlp_backward(x, dL/dy) -- what the
    create_graph branches of FusedMLPFunction / FusedMLPHalfFunction return (bit-identical to their first-order dL/dx).
    args: desc, packed (fp32, with_backward), has_bias, need (needs_input_grad of x, W_0, b_0, ...: None for the others), x, dL_dy,
    then the parameters that exist (W_0, b_0 if any, W_1, ...).

    backward: the fused double backward (nr3d_mlp_backward_backward) when ONLY dL/dx receives a gradient (the eikonal term), no
    third order is asked for (grad mode off) and desc.second_order_fusable -- dL/dW_l from the kernel, dL/db_l zeros (views of the
    same pool, as the torch route's), dL/d(dL/dy) when asked for, and None for x: its gradient is zero (piecewise linear network), and
    an [n, in] tensor of zeros would cost a full write for nothing -- so x.grad stays None when the eikonal term is x's only
    consumer.  Softplus hidden layers (FUSED_SOFTPLUS_SECOND_ORDER, desc.softplus_second_order_fusable) take
    nr3d_mlp_softplus_backward_backward under the same conditions: not piecewise linear, so x (when it needs one) and the hidden
    biases DO get a gradient from the eikonal term.  Every other case differentiates the layer-by-layer torch evaluation of the
    network, as the route before this one."""

    @staticmethod
    def _params(has_bias, flat):
        it = iter(flat)
        ws, bs = [], []
        for hb in has_bias:
            ws.append(next(it))
            bs.append(next(it) if hb else None)
        return ws, bs

    @staticmethod
    def forward(ctx, desc, packed, has_bias, need, x, dL_dy, *flat):
        from nr3d_lib_amd.bindings import _mlp
        ctx.set_materialize_grads(False)
        dx, dWs, dbs = _mlp.backward(desc, x, dL_dy, packed, need_dx=need[0], has_bias=list(has_bias))
        ctx.save_for_backward(x, dL_dy, packed, *flat)
        ctx.desc, ctx.has_bias = desc, list(has_bias)
        out = [dx]
        for l in range(len(has_bias)):
            out += [dWs[l] if need[1 + 2 * l] else None, dbs[l] if (dbs[l] is not None and need[2 + 2 * l]) else None]
        ctx.produced = [o is not None for o in out]
        return tuple(out)

    @staticmethod
    def backward(ctx, *grads):
        from nr3d_lib_amd.bindings import _mlp
        x, dL_dy, packed, *flat = ctx.saved_tensors
        if all(g is None for g in grads):
            return (None,) * (6 + len(flat))
        need_gy, need_p = ctx.needs_input_grad[5], ctx.needs_input_grad[6:]
        if (grads[0] is not None and all(g is None for g in grads[1:]) and not torch.is_grad_enabled()
                and ctx.desc.second_order_fusable):
            dgy, dWs, dbs = _mlp.backward_backward(ctx.desc, x, dL_dy, grads[0].float(), packed, need_dgy=need_gy,
                                                   has_bias=ctx.has_bias)
            # b_l reaches dL/dx only through the ReLU masks of layer l and above: zeros where the torch route has them, None where it
            # has no path (a network without ReLU behind layer l)
            n_l, relu = len(ctx.has_bias), _mlp.ACT_RELU
            gp = []
            for l, hb in enumerate(ctx.has_bias):
                reach = ctx.desc.output_activation == relu or (l + 1 < n_l and ctx.desc.hidden_activation == relu)
                gp += [dWs[l], dbs[l] if reach else None] if hb else [dWs[l]]
            return (None, None, None, None, None, dgy, *[g if n else None for g, n in zip(gp, need_p)])
        if (grads[0] is not None and all(g is None for g in grads[1:]) and not torch.is_grad_enabled()
                and FUSED_SOFTPLUS_SECOND_ORDER and ctx.desc.softplus_second_order_fusable):
            dgy, dx, dWs, dbs = _mlp.backward_backward_softplus(ctx.desc, x, dL_dy, grads[0].float(), packed, need_dgy=need_gy,
                                                                need_dx=ctx.needs_input_grad[4], has_bias=ctx.has_bias)
            # hidden biases: the kernel's sums; the output bias reaches dL/dx only through an output ReLU's mask (zeros), else not at all
            n_l, gp = len(ctx.has_bias), []
            for l, hb in enumerate(ctx.has_bias):
                reach = l + 1 < n_l or ctx.desc.output_activation == _mlp.ACT_RELU
                gp += [dWs[l], dbs[l] if reach else None] if hb else [dWs[l]]
            return (None, None, None, None, dx, dgy, *[g if n else None for g, n in zip(gp, need_p)])
        return (None, None, None, None, *FusedMLPBackwardFunction._torch_backward(ctx, x, dL_dy, flat, grads))

    @staticmethod
    def _torch_backward(ctx, x, dL_dy, flat, grads):
        """gradients of sum_k <output_k, grads_k> w.r.t. (x, dL_dy, *flat) through the layer-by-layer torch evaluation of the first
        backward.  x and dL_dy enter as detached leaves: both are downstream of the parameters (dL_dy of a loss on y), and a gradient
        taken through the originals would run into their graph -- counting the parameters' path through them a second time (the
        engine propagates the dL_dy gradient returned here itself) and freeing that graph.  Third order (grad mode on): the result is
        differentiable w.r.t. the parameters; terms through x vanish for the piecewise linear (ReLU / linear) networks -- for
        softplus hidden layers they do not, and x gets its gradient below like any other input --, terms through dL_dy are not propagated."""
        from nr3d_lib_amd.bindings import _mlp
        create = torch.is_grad_enabled()
        need_x, need_gy = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        with torch.enable_grad():
            xi = x.detach().requires_grad_(True)
            gi = dL_dy.detach().requires_grad_(need_gy)
            ws, bs = FusedMLPBackwardFunction._params(ctx.has_bias, flat)
            h = xi
            for l, (W, b) in enumerate(zip(ws, bs)):
                h = torch.nn.functional.linear(h, W, b)
                h = _torch_activation(h, ctx.desc, l + 1 < len(ws))
            slots = [xi]
            for W, b in zip(ws, bs):
                slots += [W, b]
            # the first backward's outputs that exist and receive a gradient, as functions of x, the parameters and dL/dy
            idx = [k for k, (p, g) in enumerate(zip(ctx.produced, grads)) if p and g is not None]
            firsts = torch.autograd.grad(h, [slots[k] for k in idx], gi, create_graph=True, allow_unused=True)
            pairs = [(f, grads[k]) for f, k in zip(firsts, idx) if f is not None]
            inputs = [xi, gi, *flat]
            wanted = [k for k, n in enumerate(ctx.needs_input_grad[4:]) if n]
            got = [None] * len(inputs)
            if pairs and wanted:
                res = torch.autograd.grad([f for f, _ in pairs], [inputs[k] for k in wanted], [g for _, g in pairs],
                                          create_graph=create, allow_unused=True)
                for k, r in zip(wanted, res):
                    got[k] = r
        if not need_x:
            got[0] = None
        return got


class MLP(nn.Module):
    def __init__(self, in_features: int, out_features: int, *, D: int = 4, W: Union[int, List[int]] = 128, skips: List[int] = [],
                 activation: Union[str, dict] = 'relu', output_activation: Union[str, dict] = None, bias=True,
                 last_bias: bool = None, equal_lr=False, weight_norm=False, dtype: Union[str, torch.dtype] = None,
                 device: torch.device = None):
        super().__init__()
        self.dtype = dtype = (dtype if isinstance(dtype, torch.dtype) or dtype is None
                              else getattr(torch, str(dtype).replace('torch.', '')))
        nl, gain, init_fn, first_init_fn = get_nonlinearity(activation)
        last_nl, last_gain, last_init_fn, _ = get_nonlinearity(output_activation)
        if last_bias is None:
            last_bias = bias
        self.D = D
        self.Ws = [W] * D if isinstance(W, int) else W
        if self.D >= 1:
            assert len(self.Ws) == D, f"The length of list W={self.Ws} should be D={D}."
        self.in_features, self.out_features = in_features, out_features
        self.skips, self.activation, self.output_activation = skips, activation, output_activation
        layers = []
        for l in range(self.D + 1):
            out_dim = out_features if l == self.D else self.Ws[l]
            in_dim = in_features if l == 0 else (in_features + self.Ws[l - 1] if l in self.skips else self.Ws[l - 1])
            last = l == self.D
            layer = DenseLayer(in_dim, out_dim, activation=last_nl if last else nl, bias=last_bias if last else bias,
                               dtype=self.dtype or torch.float, device=device, equal_lr=equal_lr)
            layer.apply(last_init_fn if last else (first_init_fn if l == 0 else init_fn))
            if weight_norm:
                layer = nn.utils.weight_norm(layer)
            layers.append(layer)
        self.layers = nn.ModuleList(layers)
        self._plain = not (skips or weight_norm or equal_lr)
        self._desc = None

    @property
    def device(self) -> torch.device:
        return self.layers[0].weight.device

    def invalidate_packed(self):
        """drop the cached MFMA-ordered weight copy (see CACHE_PACKED): call after editing parameters through `.data`"""
        if self._desc:
            self._desc._packed_cache = None

    def train(self, mode: bool = True):
        self.invalidate_packed()
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_packed()
        return out

    def get_weight_reg(self, norm_type: float = 2.0):
        return torch.stack([p.norm(p=norm_type) for n, p in self.layers.named_parameters()])

    # ---- the fused path ------------------------------------------------------------------------------------------------
    @staticmethod
    def _act_code(layer):
        from nr3d_lib_amd.bindings import _mlp
        """ACT_* of the layer's activation, or None when the fused kernels do not take it.  nn.Softplus fuses with threshold 20 and
        beta >= FUSED_SOFTPLUS_MIN_BETA (5.0): the line at which get_nonlinearity already treats softplus as ReLU-like, far below the
        beta = 100 of every softplus in the reference; the default beta = 1 deliberately stays on the torch path."""
        a = layer.activation
        if a is None:
            return _mlp.ACT_NONE
        if isinstance(a, nn.Softplus):
            return _mlp.ACT_SOFTPLUS if (a.threshold == 20 and a.beta >= FUSED_SOFTPLUS_MIN_BETA) else None
        if isinstance(a, nn.Sigmoid):
            return _mlp.ACT_SIGMOID          # (the output layer only: fused_desc)
        return _mlp.ACT_RELU if isinstance(a, nn.ReLU) else None

    def fused_desc(self):
        """the kernel-side description of this network, or None when the fused kernels do not apply to it"""
        if self._desc is None:
            from nr3d_lib_amd.bindings import _mlp
            ok = self._plain and self.D >= 1 and self.dtype in (None, torch.float32, torch.float16)
            hid = {self._act_code(l) for l in self.layers[:-1]}
            out = self._act_code(self.layers[-1])
            # softplus: hidden layers only, and all of them with one beta; sigmoid: the output layer only
            betas = {float(l.activation.beta) for l in self.layers[:-1] if isinstance(l.activation, nn.Softplus)}
            ok = ok and out != _mlp.ACT_SOFTPLUS and _mlp.ACT_SIGMOID not in hid and len(betas) <= 1
            if ok and len(hid) == 1 and None not in hid and out is not None and len(self.layers) <= _mlp.MAX_LAYERS:
                d = _mlp.MLPDesc([self.in_features, *self.Ws, self.out_features], hid.pop(), out, beta=betas.pop() if betas else 1.0)
                self._desc = d if (d.half_fusable if self.dtype == torch.float16 else d.fusable) else False
            else:
                self._desc = False
        return self._desc or None

    def _fused_ok(self, x, return_last, input_max_channel):
        half = self.dtype == torch.float16        # dtype=half: the layers run under autocast in the reference -> the f16-MFMA kernels
        if not (USE_FUSED and x.is_cuda and (x.dtype == torch.float32 or (half and x.dtype == torch.float16))
                and not return_last and input_max_channel is None):
            return None
        if torch.is_autocast_enabled():
            return None
        desc = self.fused_desc()
        if desc is None:
            return None
        self._needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.layers.parameters()))
        return desc if (not self._needs_grad or (desc.half_backward_fusable if half else desc.backward_fusable)) else None

    def forward_columns(self, x: torch.Tensor, n_cols: int):
        """The first ``n_cols`` output columns (fp32: contiguous) -- for queries that need a few numbers per sample and no
        gradient (the density column of a pruning query: nr3d_lib/graphics/nerf/nerf_ray_query.py:105-127 slices it out of the
        full output).  On the fused path the SAME kernels run on the network whose last layer is cut to its first rows: the columns
        they compute are bit-identical (every output column is its own dot product), the other 4 (out - n_cols) bytes per sample
        are neither written nor read back through a strided view (6.9 M samples x 16 outputs: 0.44 GB each way).  With a gradient in
        play, or off the fused path: ``self(x)[..., :n_cols]``."""
        n_cols = int(n_cols)
        desc = None
        if n_cols < self.out_features and not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.layers.parameters()))):
            desc = self._fused_ok(x, False, None)
        if desc is None:
            return self(x)[..., :n_cols]
        from nr3d_lib_amd.bindings import _mlp
        # (the half kernels store rows of whole 8-byte pieces on their fast path: four columns at least there, the view below drops the rest)
        n_keep = n_cols
        if self.dtype == torch.float16:
            n_cols = min(self.out_features, (n_cols + 3) // 4 * 4)
        sub = _mlp.MLPDesc([self.in_features, *self.Ws, n_cols], desc.hidden_activation, desc.output_activation, beta=desc.beta)
        params = []
        for layer in self.layers[:-1]:
            params += [layer.weight, layer.bias]
        last = self.layers[-1]
        params += [last.weight[:n_cols], None if last.bias is None else last.bias[:n_cols]]
        fn = FusedMLPHalfFunction if self.dtype == torch.float16 else FusedMLPFunction
        with torch.no_grad():
            return fn.apply(sub, False, x, *params)[..., :n_keep]

    @profile
    def forward(self, x: torch.Tensor, return_last: bool = False, input_max_channel: int = None):
        desc = self._fused_ok(x, return_last, input_max_channel)
        if desc is not None:
            params = []
            for layer in self.layers:
                params += [layer.weight, layer.bias]
            fn = FusedMLPHalfFunction if self.dtype == torch.float16 else FusedMLPFunction
            return fn.apply(desc, self._needs_grad, x, *params)
        # layer-by-layer path: layer 0 may see a truncated input, skip layers see [h, x], the input of the output layer
        # (index D) is what return_last hands back
        h, last_h = self.layers[0](x, max_channel=input_max_channel), None
        for i in range(1, len(self.layers)):
            if i == self.D and i not in self.skips:
                last_h = h
            h = self.layers[i](torch.cat([h, x], dim=-1) if i in self.skips else h)
        return (h, last_h) if return_last else h


FCBlock = MLP


class LipschitzNormalizeFunction(torch.autograd.Function):
    """(c, W_0 ... W_D) -> (W~_0 ... W~_D), W~_l = W_l softplus(c_l) / max(row abs-sum, softplus(c_l)): ``LipshitzMLP.normalization`` of every
    layer in ONE launch (nr3d_mlp_lipschitz_normalize), its gradient in one more (nr3d_mlp_lipschitz_normalize_backward: dL/dW_l and dL/dc
    written in a fixed order, no atomics).  fp32 GPU tensors.  Differentiable once: in an eikonal step the decoder's double backward
    produces dL/dW~, and the normalisation is differentiated once after it."""

    @staticmethod
    def forward(ctx, c, *weights):
        from nr3d_lib_amd.bindings import _mlp
        ctx.save_for_backward(c, *weights)
        return tuple(_mlp.lipschitz_normalize(weights, c))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        from nr3d_lib_amd.bindings import _mlp
        c, *ws = ctx.saved_tensors
        gs = [torch.zeros_like(w) if g is None else g.float() for g, w in zip(grads, ws)]
        dWs, dc = _mlp.lipschitz_normalize_backward(ws, c, gs)
        need = ctx.needs_input_grad
        return (dc if need[0] else None, *[dW if n else None for dW, n in zip(dWs, need[1:])])


class LipshitzMLP(MLP):
    """``LipshitzMLP`` (nr3d_lib/models/blocks/mlp.py:168-249; https://arxiv.org/abs/2202.08345): an MLP whose layers run on weights
    normalised to a learnable per-layer bound softplus(c_l) of their inf-norm, c = ``lipshitz_bound_per_layer`` (fp32, initialised to
    max_r sum_j |W[r, j]| * ``c_init_factor`` per layer).  Same constructor, parameter names and methods as the reference's.

    On the GPU (``FUSED_LIPSHITZ``) the normalised weights of all layers come from one launch (``LipschitzNormalizeFunction``) and are then
    handed, in place of the raw weights, to the routes of ``MLP``: the fused decoder kernels wherever ``MLP`` would fuse the same network
    (first and second order, ReLU / softplus hidden layers, sigmoid output, fp32 and half), the layer-by-layer torch evaluation otherwise
    (``return_last``, shapes outside the kernels, autocast).  CPU tensors, or the switch off, take the reference's torch chain."""

    def __init__(self, in_features: int, out_features: int, *, c_init_factor: float = 1.0, D: int = 4, W: Union[int, List[int]] = 128,
                 skips: List[int] = [], activation: Union[str, dict] = 'relu', output_activation: Union[str, dict] = None, bias=True,
                 last_bias: bool = None, weight_norm=False, equal_lr=False, dtype: Union[str, torch.dtype] = None,
                 device: torch.device = None):
        assert len(skips) == 0 and not weight_norm and not equal_lr
        super().__init__(in_features, out_features, D=D, W=W, skips=[], activation=activation, output_activation=output_activation,
                         bias=bias, last_bias=last_bias, equal_lr=False, weight_norm=False, dtype=dtype, device=device)
        self.lipshitz_bound_per_layer = nn.Parameter(self.initial_bounds(c_init_factor), requires_grad=True)
        self._normalized_cache = None

    @torch.no_grad()
    def initial_bounds(self, c_init_factor: float = 1.0) -> torch.Tensor:
        """the constructor's value of ``lipshitz_bound_per_layer`` for the present weights: their inf-norm times ``c_init_factor``
        (2.0 in permuto-SDF, 1.0 in the original Lipschitz regularisation)"""
        c = [layer.weight.abs().sum(dim=1).max().item() * c_init_factor for layer in self.layers]
        return torch.tensor(c, dtype=torch.float, device=self.layers[0].weight.device)

    def normalization(self, w: torch.Tensor, softplus_ci: torch.Tensor):
        absrowsum = w.abs().sum(dim=1)          # inf-norm of the matrix
        # first clamp, then divide: safe where absrowsum is tiny
        scale = softplus_ci / absrowsum.clamp_min_(softplus_ci.data)
        return w * scale[:, None]

    def lipshitz_bound_full(self):
        return torch.prod(torch.nn.functional.softplus(self.lipshitz_bound_per_layer))

    def get_weight_reg(self, norm_type: float = 2.0):
        # (without `lipshitz_bound_per_layer`)
        return torch.stack([p.norm(p=norm_type) for n, p in self.layers.named_parameters()])

    def invalidate_packed(self):
        self._normalized_cache = None
        super().invalidate_packed()

    def _normalized_weights(self):
        """[W~_l] of all layers from one launch.  CACHE_PACKED: reused while no gradient is in play and (W_l, c) are the tensors and versions
        they were computed from -- an optimiser step on c alone is a new version.  Fresh W~ are new tensors whose addresses the
        allocator may hand out again, so the packed copy keyed on them (FusedMLPFunction) is dropped whenever they are recomputed."""
        c, ws = self.lipshitz_bound_per_layer, [layer.weight for layer in self.layers]
        reuse = CACHE_PACKED and not (torch.is_grad_enabled() and (c.requires_grad or any(w.requires_grad for w in ws)))
        if reuse:
            key = tuple((p.data_ptr(), p._version) for p in (c, *ws))
            if self._normalized_cache is not None and self._normalized_cache[0] == key:
                return self._normalized_cache[1]
        self.invalidate_packed()
        out = list(LipschitzNormalizeFunction.apply(c, *ws))
        if reuse:
            self._normalized_cache = (key, out)
        return out

    def _kernel_ok(self, x):
        """does the normalisation run through the kernel?  fp32 parameters on x's GPU, within the entry's range"""
        from nr3d_lib_amd.bindings import _mlp
        c = self.lipshitz_bound_per_layer
        return (FUSED_LIPSHITZ and x.is_cuda and c.is_cuda and c.dtype == torch.float32 and len(self.layers) <= _mlp.LIPSCHITZ_MAX_LAYERS
                and all(l.weight.dtype == torch.float32 and l.weight.device == c.device and max(l.weight.shape) <= _mlp.LIPSCHITZ_MAX_DIM
                        and min(l.weight.shape) >= 1 for l in self.layers))

    def _fused_ok(self, x, return_last, input_max_channel):
        desc = super()._fused_ok(x, return_last, input_max_channel)
        if desc is not None and not self._needs_grad and torch.is_grad_enabled() and self.lipshitz_bound_per_layer.requires_grad:
            self._needs_grad = True             # the bounds alone ask for a gradient: the normalised weights do
            half = self.dtype == torch.float16
            return desc if (desc.half_backward_fusable if half else desc.backward_fusable) else None
        return desc

    def forward_columns(self, x: torch.Tensor, n_cols: int):
        return self(x)[..., :int(n_cols)]

    @profile
    def forward(self, x: torch.Tensor, return_last: bool = False):
        if not self._kernel_ok(x):
            weights = [self.normalization(layer.weight, torch.nn.functional.softplus(self.lipshitz_bound_per_layer[i]))
                       for i, layer in enumerate(self.layers)]
        else:
            weights = self._normalized_weights()
            desc = self._fused_ok(x, return_last, None)
            if desc is not None:
                params = []
                for w, layer in zip(weights, self.layers):
                    params += [w, layer.bias]
                fn = FusedMLPHalfFunction if self.dtype == torch.float16 else FusedMLPFunction
                return fn.apply(desc, self._needs_grad, x, *params)
        # layer by layer on the normalised weights (the reference's forward; autocast as DenseLayer's)
        h, last_h = x, None
        low_precision = self.dtype in (torch.float16, torch.bfloat16)
        for i, (weight, layer) in enumerate(zip(weights, self.layers)):
            with torch.autocast(device_type='cuda', dtype=self.dtype, enabled=low_precision):
                if i == self.D:
                    last_h = h
                h = torch.nn.functional.linear(h, weight, layer.bias)
                if layer.activation is not None:
                    h = layer.activation(h)
        return (h, last_h) if return_last else h


class MLPNet(MLP):
    """``MLP`` behind an input embedder (nr3d_lib/models/blocks/mlp.py:130-165): ``embed_cfg`` goes to ``get_embedder``, the network
    takes the embedded width.  The embedding is a contiguous fp32 tensor, so the block still runs on the fused decoder kernels."""

    def __init__(self, in_features: int, out_features: int, *, embed_cfg: dict = {'type': 'identity'}, D: int = 4,
                 W: Union[int, List[int]] = 128, skips: List[int] = [], activation: Union[str, dict] = 'relu',
                 output_activation: Union[str, dict] = None, weight_norm=False, dtype: Union[str, torch.dtype] = None,
                 device: torch.device = None):
        embedder, embedded_in_ch = get_embedder(embed_cfg, in_features)
        super().__init__(embedded_in_ch, out_features, D=D, W=W, skips=skips, activation=activation, output_activation=output_activation,
                         weight_norm=weight_norm, dtype=dtype, device=device)
        self.embedder = embedder

    def forward(self, x: torch.Tensor, return_last: bool = False):
        return super().forward(self.embedder(x), return_last=return_last)
