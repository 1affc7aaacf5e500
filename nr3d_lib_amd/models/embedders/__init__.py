"""Input embedders -- counterpart of nr3d_lib/models/embedders: ``get_embedder`` and the modules it builds."""
from typing import Tuple

import torch.nn as nn

from .sinusoidal_pytorch import *  # noqa: F401,F403
from .sinusoidal_cuda import *  # noqa: F401,F403
from .spherical_harmonics import *  # noqa: F401,F403


def get_embedder(embed_cfg: dict, input_dim=3, use_tcnn_backend=None) -> Tuple[nn.Module, int]:
    """(module, n_encoded_dims) for embed_cfg['type'] in none / identity / spherical / sinusoidal / sinusoidal_legacy; the other
    entries of the dict are the module's constructor arguments.  The module carries its type as ``_embedder_type``.
    ``use_tcnn_backend`` (argument or dict entry) raises: tiny-cuda-nn's encodings are not ported, and its 'spherical' expects
    inputs in [0, 1] -- it is not the same function as SHEncoder."""
    cfg = dict(embed_cfg)
    tcnn = cfg.pop('use_tcnn_backend', bool(use_tcnn_backend))
    tp = cfg.pop('type')
    if tp in ('none', 'identity'):
        enc, n_out = nn.Identity(), input_dim
    elif tcnn:
        raise NotImplementedError("nr3d_lib_amd: use_tcnn_backend=True embedders (tiny-cuda-nn encodings) are not ported; "
                                  "drop the flag to use the HIP embedders")
    elif tp == 'spherical':
        enc = SHEncoder(input_dim=input_dim, **cfg)
        n_out = enc.out_features
    elif tp == 'sinusoidal':
        enc = FreqEncoder(input_dim=input_dim, **cfg)
        n_out = enc.out_features
    elif tp == 'sinusoidal_legacy':
        enc, n_out = get_sinusoidal_embedder(input_dim=input_dim, **cfg)
    else:
        raise RuntimeError(f"[pytorch backend] Unsupported embeder type={tp}")
    enc._embedder_type = tp
    return enc, n_out
