"""ctypes front of the fused fully-connected decoder (include/nr3d_hip.h: nr3d_mlp_*).  No reference pybind module
corresponds to it -- the reference's MLP (nr3d_lib/models/blocks/mlp.py) is plain torch, its fused option is
tiny-cuda-nn (nr3d_lib/models/tcnn_adapter.py); this is the kernel side of ``nr3d_lib_amd.models.blocks.MLP``."""
import ctypes as C

import torch

from .. import _hip as H

MAX_LAYERS = 8
ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_SIGMOID = 0, 1, 2, 3


class _CDesc(C.Structure):
    _fields_ = [("n_layers", C.c_uint32), ("dims", C.c_uint32 * (MAX_LAYERS + 1)), ("hidden_activation", C.c_uint32),
                ("output_activation", C.c_uint32), ("softplus_beta", C.c_float)]


class MLPDesc:
    """dims = [in_features, hidden..., out_features]; beta: of ``hidden_activation=ACT_SOFTPLUS`` (torch.nn.Softplus(beta,
    threshold=20) after every hidden layer; forward and first backward of both precisions; its fused double backward is
    backward_backward_softplus, ``softplus_second_order_fusable``), not read otherwise.  ``output_activation=ACT_SIGMOID``: 1 / (1 + exp(-z))
    on the output layer (output only; forward and first backward of both precisions; neither double backward takes it: both
    ``..._second_order_fusable`` are False).  Any other code, sigmoid hidden or softplus output: every size is 0, nothing is fusable"""

    def __init__(self, dims, hidden_activation=ACT_RELU, output_activation=ACT_NONE, beta=1.0):
        self.dims = [int(d) for d in dims]
        self.hidden_activation, self.output_activation = int(hidden_activation), int(output_activation)
        self.beta = float(beta)
        c = _CDesc()
        n_layers = len(self.dims) - 1
        c.n_layers = n_layers if 1 <= n_layers <= MAX_LAYERS else 0
        for i, d in enumerate(self.dims[:MAX_LAYERS + 1]):
            c.dims[i] = d
        c.hidden_activation, c.output_activation = self.hidden_activation, self.output_activation
        c.softplus_beta = self.beta if self.hidden_activation == ACT_SOFTPLUS else 0.0
        self._c = c
        l = H.lib()
        self.packed_floats = l.nr3d_mlp_packed_floats(C.byref(c)) if c.n_layers else 0
        self.backward_floats = l.nr3d_mlp_backward_packed_floats(C.byref(c)) if self.packed_floats else 0
        # the half-precision twin (csrc/mlp_half.hip, f16 MFMA): sizes in bytes
        self.half_packed_bytes = l.nr3d_mlp_half_packed_bytes(C.byref(c)) if c.n_layers else 0
        self.half_backward_bytes = l.nr3d_mlp_half_backward_packed_bytes(C.byref(c)) if self.half_packed_bytes else 0
        # the fused double backward (nr3d_mlp_backward_backward) on the fp32 packed buffer
        self.second_order_ok = bool(l.nr3d_mlp_backward_backward_ok(C.byref(c))) if self.backward_floats else False
        # ... of softplus hidden layers (nr3d_mlp_softplus_backward_backward): an entry, a kernel and a launch plan of their own
        self.softplus_second_order_ok = bool(l.nr3d_mlp_softplus_backward_backward_ok(C.byref(c))) if self.backward_floats else False

    @property
    def fusable(self) -> bool:
        return self.packed_floats > 0

    @property
    def backward_fusable(self) -> bool:
        return self.backward_floats > 0

    @property
    def second_order_fusable(self) -> bool:
        return self.second_order_ok

    @property
    def softplus_second_order_fusable(self) -> bool:
        return self.softplus_second_order_ok

    @property
    def half_fusable(self) -> bool:
        return self.half_packed_bytes > 0

    @property
    def half_backward_fusable(self) -> bool:
        return self.half_backward_bytes > 0


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def _pack(desc: MLPDesc, weights, biases, with_backward, half):
    name, dtype = ("mlp.pack_half", torch.float16) if half else ("mlp.pack", torch.float32)
    if not (desc.half_fusable if half else desc.fusable):
        raise RuntimeError(f"{name}: network outside the fused kernels' range")
    dev = weights[0].device
    H.require_gpu(*weights)
    ws = [w.detach().to(dtype).contiguous() for w in weights]
    bs = [None if b is None else b.detach().to(dtype).contiguous() for b in biases]
    for l, w in enumerate(ws):
        if tuple(w.shape) != (desc.dims[l + 1], desc.dims[l]):
            raise RuntimeError(f"{name}: weights[{l}] has shape {list(w.shape)}, expected {[desc.dims[l + 1], desc.dims[l]]}")
    if with_backward and not (desc.half_backward_fusable if half else desc.backward_fusable):
        raise RuntimeError(f"{name}: the fused backward does not apply to this network")
    if half:
        packed = H.empty(desc.half_packed_bytes + (desc.half_backward_bytes if with_backward else 0), dtype=torch.uint8, device=dev)
    else:
        packed = H.empty(desc.packed_floats + (desc.backward_floats if with_backward else 0), dtype=torch.float32, device=dev)
    entry = H.lib().nr3d_mlp_half_pack if half else H.lib().nr3d_mlp_pack
    with H.on_device(dev):
        H.check(entry(C.byref(desc._c), _ptr_array(ws), _ptr_array(bs), H.ptr(packed), int(with_backward), H.stream_of(packed)))
    return packed


def pack(desc: MLPDesc, weights, biases, with_backward=False) -> torch.Tensor:
    """weights[l] [dims[l+1], dims[l]], biases[l] [dims[l+1]] | None (fp32, contiguous, on one GPU) -> packed buffer"""
    return _pack(desc, weights, biases, with_backward, half=False)


def _layout(t2: torch.Tensor):
    """[n, w] tensor -> (tensor, row stride, feature stride) the kernels can read in place: row-major (rows may be strided)
    or feature-major ([w, n] storage viewed as [n, w], what the LoTD forward returns); anything else is copied"""
    n, w = t2.shape
    if w == 1 or t2.stride(1) == 1:
        return t2, (t2.stride(0) if n > 1 else w), 1
    if n > 1 and t2.stride(0) == 1:
        return t2, 1, t2.stride(1)
    return t2.contiguous(), w, 1


def _rows(g2: torch.Tensor):
    """[n, w] dL_dy -> (tensor, row stride): rows with any row stride are read in place, anything else is copied"""
    g2 = g2 if (g2.stride(-1) == 1 or g2.shape[1] == 1) else g2.contiguous()
    return g2, (g2.stride(0) if g2.shape[0] > 1 else g2.shape[1])


def _grad_pool(desc: MLPDesc, has_bias, dev):
    """([dL_dW_l], [dL_db_l | None]) the kernels ADD their workgroups' partial sums into (one atomic per element and workgroup):
    views of ONE zero-filled fp32 buffer -- one fill launch instead of 2 per layer"""
    n_layers = len(desc.dims) - 1
    sizes = [desc.dims[l + 1] * desc.dims[l] for l in range(n_layers)] + [desc.dims[l + 1] if has_bias[l] else 0 for l in range(n_layers)]
    parts = torch.zeros(sum(sizes), dtype=torch.float32, device=dev).split(sizes)
    dWs = [parts[l].view(desc.dims[l + 1], desc.dims[l]) for l in range(n_layers)]
    return dWs, [parts[n_layers + l] if has_bias[l] else None for l in range(n_layers)]


def _forward(desc: MLPDesc, x, packed, half):
    name, dtype, what = ("mlp.forward_half", torch.float16, "half") if half else ("mlp.forward", torch.float32, "fp32")
    H.require_gpu(x, packed)
    if x.dtype != dtype or x.shape[-1] != desc.dims[0]:
        raise RuntimeError(f"{name}: expected {what} input with {desc.dims[0]} features, got {x.dtype} {list(x.shape)}")
    x2, xs, xf = _layout(x.reshape(-1, x.shape[-1]))
    n = x2.shape[0]
    y = H.empty((n, desc.dims[-1]), dtype=dtype, device=x.device)
    entry = H.lib().nr3d_mlp_half_forward if half else H.lib().nr3d_mlp_forward
    with H.on_device(x.device):
        H.check(entry(C.byref(desc._c), n, H.ptr(x2), xs, xf, H.ptr(packed), H.ptr(y), y.shape[1], H.stream_of(x)))
    return y.view(*x.shape[:-1], desc.dims[-1])


def forward(desc: MLPDesc, x: torch.Tensor, packed: torch.Tensor) -> torch.Tensor:
    """x [..., in] fp32 (row-major with any row stride, or feature-major) -> y [..., out]"""
    return _forward(desc, x, packed, half=False)


def _backward(desc: MLPDesc, x, dL_dy, packed, need_dx, has_bias, half):
    name, dtype, what = ("mlp.backward_half", torch.float16, "half") if half else ("mlp.backward", torch.float32, "fp32")
    H.require_gpu(x, dL_dy, packed)
    x2 = x.reshape(-1, desc.dims[0])
    g2 = dL_dy.reshape(-1, desc.dims[-1])
    if x2.dtype != dtype or g2.dtype != dtype or x2.shape[0] != g2.shape[0]:
        raise RuntimeError(f"{name}: expected {what} x [n, in] and dL_dy [n, out]")
    x2, xs, xf = _layout(x2)
    g2, gs = _rows(g2)
    n, dev = x2.shape[0], x.device
    dWs, dbs = _grad_pool(desc, [True] * (len(desc.dims) - 1) if has_bias is None else list(has_bias), dev)
    dx, gxs, gxf = None, desc.dims[0], 1
    if need_dx and xf != 1:
        dx, gxs, gxf = H.empty((desc.dims[0], n), dtype=dtype, device=dev).t(), 1, n
    elif need_dx:
        dx = H.empty((n, desc.dims[0]), dtype=dtype, device=dev)
    entry = H.lib().nr3d_mlp_half_backward if half else H.lib().nr3d_mlp_backward
    with H.on_device(dev):
        H.check(entry(C.byref(desc._c), n, H.ptr(x2), xs, xf, H.ptr(g2), gs, H.ptr(packed), H.ptr(dx), gxs, gxf, _ptr_array(dWs),
                      _ptr_array(dbs), H.stream_of(x)))
    return (None if dx is None else dx.reshape(x.shape)), dWs, dbs


def backward(desc: MLPDesc, x: torch.Tensor, dL_dy: torch.Tensor, packed: torch.Tensor, need_dx=True, has_bias=None):
    """-> (dL_dx | None, [dL_dW_l], [dL_db_l | None]); `packed` from pack(..., with_backward=True).  dL_dx has the layout
    of x: for a feature-major x (the LoTD features) it is feature-major too, which is what the LoTD parameter-gradient
    pass reads without a transposition."""
    return _backward(desc, x, dL_dy, packed, need_dx, has_bias, half=False)


def backward_backward(desc: MLPDesc, x: torch.Tensor, dL_dy: torch.Tensor, ddL_dx: torch.Tensor, packed: torch.Tensor, need_dgy=True,
                      has_bias=None):
    """The double backward: gradients of <dL/dx, ddL_dx> (dL/dx = backward()'s, a function of the parameters and dL_dy) ->
    (dL/d(dL_dy) | None, [dL/dW_l], [dL/db_l | None]).  ReLU / linear networks only (softplus hidden layers: desc.second_order_fusable is
    False, backward_backward_softplus takes them).  dL/dx and dL/db_l are zero (the network is piecewise linear): dL/dx is not
    produced, dL/db_l are zero views of the dW pool for the layers has_bias marks (default: none).  x and ddL_dx row-major with any
    row stride or feature-major, dL_dy rows with any row stride (0 included: an expanded ones); `packed` from
    pack(..., with_backward=True).  dL/d(dL_dy) has dL_dy's shape."""
    H.require_gpu(x, dL_dy, ddL_dx, packed)
    if not desc.second_order_fusable:
        raise RuntimeError("mlp.backward_backward: the fused double backward does not apply to this network")
    x2 = x.reshape(-1, desc.dims[0])
    v2 = ddL_dx.reshape(-1, desc.dims[0])
    g2 = dL_dy.reshape(-1, desc.dims[-1])
    if (x2.dtype != torch.float32 or g2.dtype != torch.float32 or v2.dtype != torch.float32 or x2.shape[0] != g2.shape[0]
            or v2.shape[0] != x2.shape[0]):
        raise RuntimeError("mlp.backward_backward: expected fp32 x [n, in], dL_dy [n, out] and ddL_dx [n, in]")
    x2, xs, xf = _layout(x2)
    v2, vs, vf = _layout(v2)
    g2, gs = _rows(g2)
    n, dev = x2.shape[0], x.device
    dWs, dbs = _grad_pool(desc, [False] * (len(desc.dims) - 1) if has_bias is None else list(has_bias), dev)
    dgy = H.empty((n, desc.dims[-1]), dtype=torch.float32, device=dev) if need_dgy else None
    with H.on_device(dev):
        H.check(H.lib().nr3d_mlp_backward_backward(
            C.byref(desc._c), n, H.ptr(x2), xs, xf, H.ptr(g2), gs, H.ptr(v2), vs, vf,
            H.ptr(packed), H.ptr(dgy), desc.dims[-1], _ptr_array(dWs), H.stream_of(x)))
    return (None if dgy is None else dgy.view(dL_dy.shape)), dWs, dbs


def backward_backward_softplus(desc: MLPDesc, x: torch.Tensor, dL_dy: torch.Tensor, ddL_dx: torch.Tensor, packed: torch.Tensor,
                               need_dgy=True, need_dx=True, has_bias=None):
    """The double backward of a network with softplus hidden layers (desc.softplus_second_order_fusable): gradients of <dL/dx, ddL_dx> ->
    (dL/d(dL_dy) | None, dL/dx | None, [dL/dW_l], [dL/db_l | None]).  Softplus is not piecewise linear, so x and the hidden biases get
    a gradient: dL/dx has the layout of x (feature-major for a feature-major x, as backward()'s); dL/db_l for the layers has_bias marks
    (default: all) -- the output layer's entry stays zero, its bias does not reach dL/dx.  Layout rules as backward_backward."""
    H.require_gpu(x, dL_dy, ddL_dx, packed)
    if desc.hidden_activation != ACT_SOFTPLUS:
        raise RuntimeError("mlp.backward_backward_softplus: softplus hidden layers only (ReLU / linear networks: backward_backward)")
    if not desc.softplus_second_order_fusable:
        raise RuntimeError("mlp.backward_backward_softplus: the fused double backward does not apply to this network")
    x2 = x.reshape(-1, desc.dims[0])
    v2 = ddL_dx.reshape(-1, desc.dims[0])
    g2 = dL_dy.reshape(-1, desc.dims[-1])
    if (x2.dtype != torch.float32 or g2.dtype != torch.float32 or v2.dtype != torch.float32 or x2.shape[0] != g2.shape[0]
            or v2.shape[0] != x2.shape[0]):
        raise RuntimeError("mlp.backward_backward_softplus: expected fp32 x [n, in], dL_dy [n, out] and ddL_dx [n, in]")
    x2, xs, xf = _layout(x2)
    v2, vs, vf = _layout(v2)
    g2, gs = _rows(g2)
    n, dev = x2.shape[0], x.device
    dWs, dbs = _grad_pool(desc, [True] * (len(desc.dims) - 1) if has_bias is None else list(has_bias), dev)
    dgy = H.empty((n, desc.dims[-1]), dtype=torch.float32, device=dev) if need_dgy else None
    dx, gxs, gxf = None, desc.dims[0], 1
    if need_dx and xf != 1:
        dx, gxs, gxf = H.empty((desc.dims[0], n), dtype=torch.float32, device=dev).t(), 1, n
    elif need_dx:
        dx = H.empty((n, desc.dims[0]), dtype=torch.float32, device=dev)
    with H.on_device(dev):
        H.check(H.lib().nr3d_mlp_softplus_backward_backward(
            C.byref(desc._c), n, H.ptr(x2), xs, xf, H.ptr(g2), gs, H.ptr(v2), vs, vf, H.ptr(packed), H.ptr(dgy), desc.dims[-1],
            H.ptr(dx), gxs, gxf, _ptr_array(dWs), _ptr_array(dbs), H.stream_of(x)))
    return (None if dgy is None else dgy.view(dL_dy.shape)), (None if dx is None else dx.reshape(x.shape)), dWs, dbs


# ------------------------------------------------------------------------------------------------
# the weight normalisation of a Lipschitz MLP (nr3d_mlp_lipschitz_normalize*, csrc/mlp_lipschitz.hip): one launch each way for all
# layers of a network -- W~_l = W_l softplus(c_l) / max(row abs-sum, softplus(c_l)); not restricted to the fused decoder's shapes
# ------------------------------------------------------------------------------------------------
LIPSCHITZ_MAX_LAYERS = MAX_LAYERS + 1
LIPSCHITZ_MAX_DIM = 4096


def _lipschitz_args(name, weights, c):
    """checks -> (contiguous weights, rows[], cols[], sizes, c, half)"""
    weights = list(weights)
    H.require_gpu(c, *weights)
    n = len(weights)
    if not 1 <= n <= LIPSCHITZ_MAX_LAYERS:
        raise RuntimeError(f"{name}: {n} layers, expected 1..{LIPSCHITZ_MAX_LAYERS}")
    dtype, dev = weights[0].dtype, weights[0].device
    if dtype not in (torch.float32, torch.float16) or any(w.dtype != dtype or w.device != dev for w in weights):
        raise RuntimeError(f"{name}: the weights must all be float32 or all be float16, on one GPU")
    if c.dtype != torch.float32 or c.device != dev or tuple(c.shape) != (n,):
        raise RuntimeError(f"{name}: expected c float32 [{n}] on the weights' device, got {c.dtype} {list(c.shape)}")
    for l, w in enumerate(weights):
        if w.dim() != 2 or not (1 <= w.shape[0] <= LIPSCHITZ_MAX_DIM and 1 <= w.shape[1] <= LIPSCHITZ_MAX_DIM):
            raise RuntimeError(f"{name}: weights[{l}] has shape {list(w.shape)}, expected [rows, cols] with both in 1..{LIPSCHITZ_MAX_DIM}")
    ws = [w.detach().contiguous() for w in weights]
    rows = (C.c_uint32 * n)(*[w.shape[0] for w in ws])
    cols = (C.c_uint32 * n)(*[w.shape[1] for w in ws])
    return ws, rows, cols, [w.numel() for w in ws], c.detach().contiguous(), dtype == torch.float16


def lipschitz_normalize(weights, c):
    """weights[l] [rows_l, cols_l] (all float32 or all float16, on one GPU), c float32 [n_layers] -> [W~_l] of the weights' dtype: views of
    ONE allocation, written by one launch"""
    ws, rows, cols, sizes, c, half = _lipschitz_args("mlp.lipschitz_normalize", weights, c)
    outs = [o.view_as(w) for o, w in zip(H.empty(sum(sizes), dtype=ws[0].dtype, device=c.device).split(sizes), ws)]
    with H.on_device(c.device):
        H.check(H.lib().nr3d_mlp_lipschitz_normalize(len(ws), rows, cols, _ptr_array(ws), int(half), H.ptr(c), _ptr_array(outs),
                                                     H.stream_of(c)))
    return outs


def lipschitz_normalize_backward(weights, c, grads):
    """grads[l] = dL/dW~_l (float32, the shapes of the weights) -> ([dL/dW_l float32], dL/dc float32 [n_layers]): views of ONE allocation,
    written (not accumulated) by one launch in a fixed summation order"""
    name = "mlp.lipschitz_normalize_backward"
    ws, rows, cols, sizes, c, half = _lipschitz_args(name, weights, c)
    grads = list(grads)
    H.require_gpu(*grads)
    if len(grads) != len(ws) or any(g.dtype != torch.float32 or g.shape != w.shape or g.device != c.device for g, w in zip(grads, ws)):
        raise RuntimeError(f"{name}: expected one float32 gradient of each weight's shape, on the weights' device")
    gs = [g.detach().contiguous() for g in grads]
    n = len(ws)
    parts = H.empty(sum(sizes) + n, dtype=torch.float32, device=c.device).split(sizes + [n])
    dWs = [p.view_as(w) for p, w in zip(parts, ws)]
    with H.on_device(c.device):
        H.check(H.lib().nr3d_mlp_lipschitz_normalize_backward(n, rows, cols, _ptr_array(ws), int(half), H.ptr(c), _ptr_array(gs),
                                                              _ptr_array(dWs), H.ptr(parts[n]), H.stream_of(c)))
    return dWs, parts[n]


# ------------------------------------------------------------------------------------------------
# half precision on the f16 MFMA (nr3d_mlp_half_*): half x / weights / y, fp32 accumulation inside a layer, activations
# rounded to half between the layers -- the contract of the reference's tcnn FullyFusedMLP (models/tcnn_adapter.py:37-51)
# ------------------------------------------------------------------------------------------------
def pack_half(desc: MLPDesc, weights, biases, with_backward=False) -> torch.Tensor:
    """weights[l] [dims[l+1], dims[l]], biases[l] [dims[l+1]] | None (half, on one GPU) -> packed byte buffer"""
    return _pack(desc, weights, biases, with_backward, half=True)


def forward_half(desc: MLPDesc, x: torch.Tensor, packed: torch.Tensor) -> torch.Tensor:
    """x [..., in] half (row-major with any row stride, or feature-major) -> y [..., out] half"""
    return _forward(desc, x, packed, half=True)


def backward_half(desc: MLPDesc, x: torch.Tensor, dL_dy: torch.Tensor, packed: torch.Tensor, need_dx=True, has_bias=None):
    """-> (dL_dx half | None, [dL_dW_l fp32], [dL_db_l fp32 | None]); `packed` from pack_half(..., with_backward=True).  The
    parameter gradients are the fp32 sums the kernel accumulated (the caller rounds them to the parameters' dtype)."""
    return _backward(desc, x, dL_dy, packed, need_dx, has_bias, half=True)
