"""Sinusoidal embedding on the HIP kernels of csrc/embed.hip -- counterpart of nr3d_lib/models/embedders/sinusoidal_cuda/freq.py
(``freq_encode``, ``FreqEncoder``), same column layout as ``SinusoidalEmbedder`` of sinusoidal_pytorch.py.

Unlike the reference's (``once_differentiable``, "Not 2nd-backwardable"), the backward here is itself a differentiable op whose
backward is one fused kernel, so ``autograd.grad(h_embed, x, g, create_graph=True)`` followed by a loss on the result works (the
eikonal step of an SDF with a sinusoidal extra embedder); third order raises.  float32 only; a CPU tensor raises (the reference moves
it to the GPU silently)."""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from nr3d_lib_amd.bindings import _freqencoder as _backend
from nr3d_lib_amd.profile import profile
from .._amp import custom_bwd, custom_fwd

__all__ = ['freq_encode', 'FreqEncoder']


class _freq_encoder(Function):
    @staticmethod
    @custom_fwd(cast_inputs=torch.float32)
    def forward(ctx, inputs, n_frequencies, output_dim):
        """inputs [B, D] -> [B, output_dim]"""
        from nr3d_lib_amd import _hip as H
        H.require_gpu(inputs)
        # freq_encode hands in a contiguous float32 tensor: a copy made HERE would not be recorded by autograd, the saved copy would
        # have no history and the double backward's dL/dx would never reach the caller's tensor
        if not inputs.is_contiguous():
            raise RuntimeError("_freq_encoder: `inputs` must be contiguous (call freq_encode, which makes it so where autograd sees it)")
        B, D = inputs.shape
        outputs = H.empty(B, output_dim, dtype=inputs.dtype, device=inputs.device)
        _backend.freq_encode_forward(inputs, B, D, n_frequencies, output_dim, outputs)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(inputs, outputs)
            ctx.dims = (B, D, n_frequencies, output_dim)
        return outputs

    @staticmethod
    @custom_bwd
    def backward(ctx, grad):
        inputs, outputs = ctx.saved_tensors
        return _freq_encoder_backward.apply(grad.contiguous(), inputs, outputs.detach(), ctx.dims), None, None


class _freq_encoder_backward(Function):
    """grad_inputs = backward(grad, outputs) as a differentiable function of ``grad`` and (through the saved outputs) ``inputs``; its
    backward is the fused double backward.  ``outputs`` comes in detached: its dependence on ``inputs`` is folded into the kernel."""

    @staticmethod
    def forward(ctx, grad, inputs, outputs, dims):
        B, D, n_frequencies, output_dim = dims
        grad_inputs = torch.empty_like(inputs)
        _backend.freq_encode_backward(grad, outputs, B, D, n_frequencies, output_dim, grad_inputs)
        ctx.save_for_backward(grad, outputs)
        ctx.dims = dims
        return grad_inputs

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        grad, outputs = ctx.saved_tensors
        B, D, n_frequencies, output_dim = ctx.dims
        d_grad = torch.empty_like(grad) if ctx.needs_input_grad[0] else None
        d_inputs = torch.empty(B, D, dtype=grad.dtype, device=grad.device) if ctx.needs_input_grad[1] else None
        _backend.freq_encode_backward_backward(v.contiguous(), grad, outputs, B, D, n_frequencies, output_dim, d_grad, d_inputs)
        return d_grad, d_inputs, None, None


def freq_encode(input: torch.Tensor, n_frequencies: int, output_dim: int = None) -> torch.Tensor:
    D = input.shape[-1]
    if output_dim is None:
        output_dim = D + 2 * D * n_frequencies
    # the cast of an autocast region and the contiguous copy happen out here, as recorded autograd ops: the Function then saves the very
    # tensor it was given, so the gradients of its double backward flow on to the caller's (sliced, transposed, half) tensor
    if input.is_cuda and torch.is_autocast_enabled() and input.is_floating_point() and input.dtype != torch.float32:
        input = input.float()
    return _freq_encoder.apply(input.contiguous(), n_frequencies, output_dim)


class FreqEncoder(nn.Module):
    def __init__(self, input_dim=3, n_frequencies=4, include_input=True):
        super().__init__()
        assert include_input, "Currently sinusoidal embedder only support `include_input`==True."
        self.in_features = input_dim
        self.n_frequencies = n_frequencies
        self.out_features = input_dim + input_dim * 2 * n_frequencies

    def __repr__(self):
        return f"FreqEncoder: input_dim={self.in_features}, output_dim={self.out_features}, n_frequencies={self.n_frequencies} "

    @profile
    def forward(self, inputs, **kwargs) -> torch.Tensor:
        """inputs [..., input_dim] -> [..., out_features]"""
        lead = inputs.shape[:-1]
        flat = inputs.reshape(-1, inputs.shape[-1])
        return freq_encode(flat, self.n_frequencies, self.out_features).reshape(*lead, self.out_features)
