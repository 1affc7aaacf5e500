"""nr3d_lib_amd.bindings._freqencoder -- drop-in for the reference pybind module ``nr3d_lib.bindings._freqencoder``
(externals/freqencoder/bindings.cpp), backed by csrc/embed.hip through include/nr3d_hip.h.

Same names, argument order and caller-allocated tensors; float32 only (the reference's ``data_ptr<float>`` refuses anything else);
``freq_encode_backward`` OVERWRITES ``grad_inputs``, as the reference's kernel does.  A CPU tensor raises RuntimeError by name.
``freq_encode_backward_backward`` is new: the reference has no second order."""
import torch

from .. import _hip as H

__all__ = ["freq_encode_forward", "freq_encode_backward", "freq_encode_backward_backward"]


def _chk(fn, **tensors):
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{fn}: `{name}` must be a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"{fn}: `{name}` must be a CUDA tensor (got a CPU tensor; there is no CPU fallback)")
        if not t.is_contiguous():
            raise RuntimeError(f"{fn}: `{name}` must be a contiguous tensor")
        if not t.dtype.is_floating_point:
            raise RuntimeError(f"{fn}: `{name}` must be a floating tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{fn}: expected scalar type Float but found {t.dtype} for `{name}`")


def _need(fn, name, t, numel):
    if t.numel() < numel:
        raise RuntimeError(f"{fn}: `{name}` holds {t.numel()} elements, {numel} are needed")


def freq_encode_forward(inputs, B, D, deg, C, outputs):
    """outputs [B, C] <- embedding of inputs [B, D] with deg frequencies, C = D + 2 D deg (freqencoder.cu:101-114)"""
    fn = "freq_encode_forward"
    B, D, deg, C = int(B), int(D), int(deg), int(C)
    _chk(fn, inputs=inputs, outputs=outputs)
    _need(fn, "inputs", inputs, B * D)
    _need(fn, "outputs", outputs, B * C)
    with H.on_device(inputs.device):
        H.check(H.lib().nr3d_freq_encode_fwd(B, D, deg, C, H.ptr(inputs), H.ptr(outputs), C, H.stream_of(inputs)))


def freq_encode_backward(grad, outputs, B, D, deg, C, grad_inputs):
    """grad_inputs [B, D] <- from grad [B, C] and the forward's outputs (freqencoder.cu:117-133)"""
    fn = "freq_encode_backward"
    B, D, deg, C = int(B), int(D), int(deg), int(C)
    _chk(fn, grad=grad, outputs=outputs, grad_inputs=grad_inputs)
    _need(fn, "grad", grad, B * C)
    _need(fn, "outputs", outputs, B * C)
    _need(fn, "grad_inputs", grad_inputs, B * D)
    with H.on_device(grad.device):
        H.check(H.lib().nr3d_freq_encode_bwd(B, D, deg, C, H.ptr(grad), H.ptr(outputs), C, H.ptr(grad_inputs), H.stream_of(grad)))


def freq_encode_backward_backward(v, grad, outputs, B, D, deg, C, d_grad, d_inputs):
    """the backward of freq_encode_backward: v = dL/d(grad_inputs) [B, D]; d_grad [B, C] | None and d_inputs [B, D] | None are
    overwritten with dL/dgrad and dL/dinputs"""
    fn = "freq_encode_backward_backward"
    B, D, deg, C = int(B), int(D), int(deg), int(C)
    _chk(fn, v=v, grad=grad, outputs=outputs, **{k: t for k, t in (("d_grad", d_grad), ("d_inputs", d_inputs)) if t is not None})
    _need(fn, "v", v, B * D)
    _need(fn, "grad", grad, B * C)
    _need(fn, "outputs", outputs, B * C)
    if d_grad is not None:
        _need(fn, "d_grad", d_grad, B * C)
    if d_inputs is not None:
        _need(fn, "d_inputs", d_inputs, B * D)
    with H.on_device(v.device):
        H.check(H.lib().nr3d_freq_encode_bwd_bwd(B, D, deg, C, H.ptr(v), H.ptr(grad), H.ptr(outputs), C, H.ptr(d_grad), H.ptr(d_inputs),
                                                 H.stream_of(v)))


def freq_encode_into(inputs, out, deg):
    """``out`` [B, C columns of a wider row-major buffer] <- embedding of inputs: the strided output of nr3d_freq_encode_fwd"""
    fn = "freq_encode_into"
    _chk(fn, inputs=inputs)
    B, D = inputs.shape
    C = D + 2 * D * int(deg)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1
            and out.shape == (B, C)):
        raise RuntimeError(f"{fn}: `out` must be a [{B}, {C}] float32 CUDA view with unit column stride")
    with H.on_device(inputs.device):
        H.check(H.lib().nr3d_freq_encode_fwd(B, D, int(deg), C, H.ptr(inputs), H.ptr(out), out.stride(0) if B > 1 else C,
                                             H.stream_of(inputs)))
    return out
