"""nr3d_lib_amd.bindings._shencoder -- drop-in for the reference pybind module ``nr3d_lib.bindings._shencoder``
(externals/shencoder/bindings.cpp), backed by csrc/embed.hip through include/nr3d_hip.h.

Same names, argument order and caller-allocated tensors: ``C`` is the DEGREE (the embedding has C^2 columns), as in the reference.

Deliberate differences:
  * half tensors are evaluated in fp32 and rounded once at the store (the reference computes them in half);
  * float64 is refused (the reference dispatches it); a CPU tensor raises RuntimeError by name;
  * ``sh_encode_backward`` takes ``dy_dx=None``: the derivatives are then recomputed from ``inputs`` instead of read back.
As in the reference, ``sh_encode_backward`` ACCUMULATES into ``grad_inputs`` (its kernel `+=`s into a zero-filled tensor).
"""
import torch

from .. import _hip as H

__all__ = ["sh_encode_forward", "sh_encode_backward"]


def _chk(fn, dtype=None, **tensors):
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{fn}: `{name}` must be a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"{fn}: `{name}` must be a CUDA tensor (got a CPU tensor; there is no CPU fallback)")
        if not t.is_contiguous():
            raise RuntimeError(f"{fn}: `{name}` must be a contiguous tensor")
        if not t.dtype.is_floating_point:
            raise RuntimeError(f"{fn}: `{name}` must be a floating tensor")
        if t.dtype not in (torch.float32, torch.float16):
            raise RuntimeError(f"{fn}: `{name}` is {t.dtype}; float32 and float16 are supported")
        if dtype is not None and t.dtype != dtype:
            raise RuntimeError(f"{fn}: `{name}` is {t.dtype}, inputs are {dtype}")


def _need(fn, name, t, numel):
    if t.numel() < numel:
        raise RuntimeError(f"{fn}: `{name}` holds {t.numel()} elements, {numel} are needed")


def sh_encode_forward(inputs, outputs, B, D, C, calc_grad_inputs, dy_dx):
    """outputs [B, C^2] <- SH(inputs [B, D = 3]) of degree C; with calc_grad_inputs also dy_dx [B, D * C^2] (shencoder.cu:406-423)"""
    fn = "sh_encode_forward"
    B, D, C = int(B), int(D), int(C)
    _chk(fn, inputs=inputs)
    _chk(fn, inputs.dtype, outputs=outputs)
    _need(fn, "inputs", inputs, B * D)
    _need(fn, "outputs", outputs, B * C * C)
    jac = None
    if calc_grad_inputs:
        _chk(fn, inputs.dtype, dy_dx=dy_dx)
        _need(fn, "dy_dx", dy_dx, B * D * C * C)
        jac = dy_dx
    with H.on_device(inputs.device):
        H.check(H.lib().nr3d_sh_encode_fwd(B, D, C, H.DTYPE_CODE[inputs.dtype], H.ptr(inputs), H.ptr(outputs), C * C, H.ptr(jac),
                                           H.stream_of(inputs)))


def sh_encode_backward(grad, inputs, B, D, C, dy_dx, grad_inputs):
    """grad_inputs [B, D] += grad [B, C^2] . dy_dx (shencoder.cu:425-445); dy_dx None: recomputed from inputs"""
    fn = "sh_encode_backward"
    B, D, C = int(B), int(D), int(C)
    _chk(fn, inputs=inputs)
    _chk(fn, inputs.dtype, grad=grad, grad_inputs=grad_inputs)
    _need(fn, "inputs", inputs, B * D)
    _need(fn, "grad", grad, B * C * C)
    _need(fn, "grad_inputs", grad_inputs, B * D)
    if dy_dx is not None:
        _chk(fn, inputs.dtype, dy_dx=dy_dx)
        _need(fn, "dy_dx", dy_dx, B * D * C * C)
    with H.on_device(inputs.device):
        H.check(H.lib().nr3d_sh_encode_bwd(B, D, C, H.DTYPE_CODE[inputs.dtype], H.ptr(grad), C * C, H.ptr(inputs), H.ptr(dy_dx),
                                           H.ptr(grad_inputs), 1, H.stream_of(inputs)))


def sh_encode_into(inputs, out, degree):
    """``out`` [B, >= degree^2 columns of a wider row-major buffer] <- SH(inputs): the strided output of nr3d_sh_encode_fwd (an
    extension: a caller can embed straight into the rows a decoder reads)"""
    fn = "sh_encode_into"
    _chk(fn, inputs=inputs)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == inputs.dtype and out.dim() == 2 and out.stride(1) == 1
            and out.shape == (inputs.shape[0], degree * degree)):
        raise RuntimeError(f"{fn}: `out` must be a [{inputs.shape[0]}, {degree * degree}] {inputs.dtype} CUDA view with unit column stride")
    B = inputs.shape[0]
    with H.on_device(inputs.device):
        H.check(H.lib().nr3d_sh_encode_fwd(B, inputs.shape[1], int(degree), H.DTYPE_CODE[inputs.dtype], H.ptr(inputs), H.ptr(out),
                                           out.stride(0) if B > 1 else degree * degree, None, H.stream_of(inputs)))
    return out
