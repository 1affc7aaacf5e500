"""what the NeuS and the NeRF ray-query drivers share (``graphics.neus.neus_ray_query``, ``graphics.nerf.nerf_ray_query``)"""
import torch


def _flag(model, name):
    return bool(getattr(model, name, False))


def _chunked(fn, kwargs: dict, chunk: int) -> torch.Tensor:
    """fn(**kwargs) evaluated on slices of at most `chunk` rows (every tensor argument is sliced along dim 0)"""
    n = next(iter(kwargs.values())).shape[0]
    if n <= chunk:
        return fn(**kwargs)
    return torch.cat([fn(**{k: v[i:i + chunk] for k, v in kwargs.items()}) for i in range(0, n, chunk)], 0)


def _march(model, ray_tested, rays_o, rays_d, near, far, perturb, march_cfg):
    """dispatch on what the accel's ray_march accepts (single / dynamic / batched / batched-dynamic accels of the
    reference differ only in the extra per-ray arguments, nerf_ray_query.py:84-104)"""
    accel = model.accel
    if hasattr(accel, 'cur_batch__ray_march'):
        extra = [ray_tested['rays_bidx']] + ([ray_tested['rays_ts']] if getattr(accel, 'is_dynamic', False) else [])
        return accel.cur_batch__ray_march(rays_o, rays_d, *extra, near=near, far=far, perturb=perturb, **march_cfg)
    if getattr(accel, 'is_dynamic', False):
        return accel.ray_march(rays_o, rays_d, ray_tested['rays_ts'], near=near, far=far, perturb=perturb, **march_cfg)
    return accel.ray_march(rays_o, rays_d, near=near, far=far, perturb=perturb, **march_cfg)
