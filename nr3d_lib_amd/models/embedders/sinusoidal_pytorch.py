"""Sinusoidal positional embeddings in plain torch -- counterpart of nr3d_lib/models/embedders/sinusoidal_pytorch.py
(``SinusoidalEmbedder``, ``AnnealedSinusoidalEmbedder``, ``get_sinusoidal_embedder``): host-side modules, provided so that
``get_embedder(type='sinusoidal_legacy')`` and annealed configurations carry over, and the CPU-runnable statement of what
csrc/embed.hip's frequency kernels compute.  Same constructor arguments, buffers (``freq_bands``, ``alpha``), column order
[x, sin(f0 x), sin(f0 x + pi/2), sin(f1 x), ...] with each block D wide, and the same fp32 arithmetic: outputs equal the reference's
bit for bit."""
import math

import torch
import torch.nn as nn

from nr3d_lib_amd.profile import profile

__all__ = ['SinusoidalEmbedder', 'AnnealedSinusoidalEmbedder', 'get_sinusoidal_embedder']

_HALF_PI = math.pi / 2.


class SinusoidalEmbedder(nn.Module):
    def __init__(self, input_dim: int, N_freqs: int, max_freq_log2: int, min_freq_log2: int = 0., log_sampling=True, include_input=True):
        """input_dim -> (input_dim if include_input) + 2 * input_dim * N_freqs columns; the bands are 2^linspace(min, max) when
        log_sampling, else linspace(2^min, 2^max)"""
        super().__init__()
        self.input_dim, self.include_input = input_dim, include_input
        self.min_freq_log2, self.max_freq_log2 = min_freq_log2, max_freq_log2
        self.out_features = (input_dim if include_input else 0) + 2 * input_dim * N_freqs
        if log_sampling:
            bands = 2. ** torch.linspace(min_freq_log2, max_freq_log2, N_freqs)
        else:
            bands = torch.linspace(2. ** min_freq_log2, 2. ** max_freq_log2, N_freqs)
        self.register_buffer('freq_bands', bands, persistent=False)

    def _angles(self, x, bands):
        """[..., N_freqs, 2, D]: band * x and band * x + pi/2 (the cosine column as a shifted sine)"""
        a = (x.unsqueeze(-2) * bands.unsqueeze(-1)).unsqueeze(-2)
        return torch.cat([a, a + _HALF_PI], dim=-2)

    @profile
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """[..., input_dim] -> [..., out_features]"""
        assert x.shape[-1] == self.input_dim
        parts = [x] if self.include_input else []
        if self.freq_bands.numel() > 0:
            parts.append(torch.sin(self._angles(x, self.freq_bands.to(x))).flatten(-3, -1))
        out = torch.cat(parts, dim=-1)
        assert out.shape[-1] == self.out_features
        return out

    def extra_repr(self) -> str:
        return f"in_dim={self.input_dim}, out_dim={self.out_features}, freq_bands=({len(self.freq_bands)}){self.freq_bands}"


class AnnealedSinusoidalEmbedder(SinusoidalEmbedder):
    """Coarse-to-fine: band k is weighted by a cosine easing window of ``alpha * N_freqs - k`` clipped to [0, 1] (nerfies), bands
    whose weight is zero give exact zeros."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.register_buffer('alpha', torch.tensor([1.0]), persistent=True)
        self.set_cosine_easing_window(self.alpha)

    @staticmethod
    def _easing(progress):
        """0 -> 0, 1 -> 1 along half a cosine period: (1 + cos(pi p + pi)) / 2 for p clipped to [0, 1]"""
        return 0.5 * (1 + torch.cos(math.pi * torch.clip(progress, 0.0, 1.0) + math.pi))

    def set_cosine_easing_window(self, alpha: float):
        """alpha in [0, 1]: 0 switches every band off, 1 all on; in between band k has progressed by alpha * N_freqs - k"""
        self.alpha[:] = alpha
        n_bands = len(self.freq_bands)
        progress = alpha * n_bands - torch.arange(n_bands)
        self.window = self._easing(progress)
        self.freq_inds = torch.nonzero(progress > 0, as_tuple=True)[0]

    @profile
    def forward(self, x: torch.Tensor):
        assert hasattr(self, 'window'), "Must call set_cosine_easing_window(alpha)"
        assert x.shape[-1] == self.input_dim
        parts = [x] if self.include_input else []
        n = len(self.freq_bands)
        if n > 0:
            window = self.window.to(device=x.device, dtype=x.dtype)
            active = torch.zeros(n, dtype=torch.bool, device=x.device)
            active[self.freq_inds.to(x.device)] = True
            ang = self._angles(x, self.freq_bands)
            feat = torch.where(active.view(n, 1, 1), torch.sin(ang) * window.view(n, 1, 1), ang.new_zeros(()))
            parts.append(feat.flatten(-3, -1))
        out = torch.cat(parts, dim=-1)
        assert out.shape[-1] == self.out_features
        return out


def get_sinusoidal_embedder(n_frequencies, input_dim=3, annealed=False):
    """(module, n_encoded_dims); n_frequencies < 0: the identity"""
    if n_frequencies < 0:
        return nn.Identity(), input_dim
    cls = AnnealedSinusoidalEmbedder if annealed else SinusoidalEmbedder
    m = cls(input_dim=input_dim, N_freqs=n_frequencies, max_freq_log2=n_frequencies - 1, log_sampling=True, include_input=True)
    return m, m.out_features
