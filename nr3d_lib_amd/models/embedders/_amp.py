"""``custom_fwd(cast_inputs=torch.float32)`` / ``custom_bwd`` for CUDA under either spelling torch offers"""
import functools

try:
    from torch.amp import custom_bwd as _bwd, custom_fwd as _fwd
    custom_fwd = functools.partial(_fwd, device_type="cuda")
    custom_bwd = functools.partial(_bwd, device_type="cuda")
except ImportError:                                     # torch < 2.4
    from torch.cuda.amp import custom_bwd, custom_fwd   # noqa: F401
