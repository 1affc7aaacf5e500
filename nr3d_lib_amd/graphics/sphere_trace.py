"""Sphere tracing through a dense occupancy grid: the Python driver of nr3d_lib_amd.bindings._sphere_trace.

Counterpart of nr3d_lib/graphics/sphere_trace.py:22-170: same constructor defaults, same ``trace(rays, sdf_query, print_debug_log,
debug_output, debug_replay)`` control flow -- segment march, ``init_rays``, then ``min(i + 1, max_steps_between_compact)`` steps
between compactions until ``max_march_iters``, ``drop_alive_rate`` or ``tail_sample_threshold`` ends the march, then the optional tail
sampling.  One step is one SDF query and ONE tracer launch (``advance_rays`` leaves the next query positions behind, which
``get_trace_positions`` returns as a view); one host wait per compaction.  Logging goes through the standard ``logging`` module
(logger ``sphere_trace``; ``print_debug_log`` switches it to DEBUG)."""
import logging
from operator import itemgetter
from typing import Any, Callable, Dict, Union

import torch

import nr3d_lib_amd.bindings._sphere_trace as _backend
from nr3d_lib_amd.profile import profile

__all__ = ["SphereTracer", "DenseGrid"]

DenseGrid = _backend.DenseGrid
logger = logging.getLogger("sphere_trace")


class SphereTracer:
    """A class for performing sphere tracing (nr3d_lib/graphics/sphere_trace.py:22-57).

    grid: ``DenseGrid(*resolution, occ_grid_tensor)``; zero_offset: SDF value that defines the surface; distance_scale: factor on the
    SDF values; min_step: smallest step along a ray; hit_threshold: ``|sdf| <=`` this is a hit; max_steps_between_compact: steps between
    two compactions of the alive rays; max_march_iters: steps at most; drop_alive_rate: stop when this share of the rays is still alive;
    tail_sample_threshold: with this many (or fewer) rays alive, stop marching and sample the rest of their segments uniformly with
    tail_sample_step_size (default min_step)."""

    def __init__(self, grid: DenseGrid, *, zero_offset: float = 0., distance_scale: float = 1., min_step: float = .1,
                 hit_threshold: float = 1e-3, max_steps_between_compact: int = 4, max_march_iters: int = 1000,
                 drop_alive_rate: float = 0., tail_sample_threshold: int = 0, tail_sample_step_size: float = None):
        self.grid = grid
        self.zero_offset = zero_offset
        self.distance_scale = distance_scale
        self.min_step = min_step
        self.max_steps_between_compact = max_steps_between_compact
        self.max_march_iters = max_march_iters
        self.drop_alive_rate = 0. if tail_sample_threshold else drop_alive_rate
        self.tail_sample_threshold = tail_sample_threshold
        self.tail_sample_step_size = tail_sample_step_size if tail_sample_step_size is not None else min_step
        self.last_march_iters = 0
        self.backend = _backend.SphereTracer(min_step, distance_scale, zero_offset, hit_threshold)

    @profile
    @torch.no_grad()
    def trace(self, rays: Dict[str, Union[int, torch.Tensor]],
              sdf_query: Callable[[torch.Tensor], Union[torch.Tensor, Dict[str, torch.Tensor]]],
              print_debug_log: bool = False, debug_output: Dict[str, Any] = None,
              debug_replay: bool = False) -> Dict[str, torch.Tensor]:
        """rays: dict with rays_o [N, 3], rays_d [N, 3], near [N], far [N]; sdf_query: positions [n, 3] -> SDF values [n] (or a dict
        with them under "sdf").  Returns the hit rays: pos [N', 3], dir [N', 3], idx [N'] (into the input rays), t [N'], n_steps [N']
        and n_rays."""
        logger.setLevel(logging.DEBUG if print_debug_log else logging.INFO)
        n_rays = rays["rays_o"].shape[0]
        n_drop_alive = self.drop_alive_rate * n_rays
        share = lambda n: n / max(n_rays, 1) * 100      # noqa: E731

        def query_sdf(pts):
            query_ret = sdf_query(pts)
            return (query_ret["sdf"] if isinstance(query_ret, dict) else query_ret).to(torch.float).contiguous()

        with profile("sphere_tracer.get_init_segments"):
            valid_rays_idx, segs_pack_info, segs, _, _ = _backend.ray_march(
                self.grid, *itemgetter("rays_o", "rays_d", "near", "far")(rays), enable_debug=False)
        n_rays_alive = valid_rays_idx.numel()
        logger.debug("Trace raymarch - %d (%.2f%%) rays alive", n_rays_alive, share(n_rays_alive))
        if debug_output is not None:
            debug_output["segs_pack_info"] = segs_pack_info
            debug_output["segs"] = segs

        with profile("sphere_tracer.init_rays"):
            self.backend.init_rays(*itemgetter("rays_o", "rays_d")(rays), valid_rays_idx, segs_pack_info, segs)
        logger.debug("Trace initial - %d (%.2f%%) rays alive", n_rays_alive, share(n_rays_alive))

        i = 0
        with profile("sphere_tracer.march"):
            while (debug_replay and i < self.last_march_iters and n_rays_alive > 0) \
                or (i < self.max_march_iters and n_rays_alive > n_drop_alive
                    and n_rays_alive > self.tail_sample_threshold):
                compact_step_size = min(i + 1, self.max_steps_between_compact)
                for _ in range(compact_step_size):
                    pts = self.backend.get_trace_positions()
                    distances = query_sdf(pts)
                    if debug_output is not None:
                        debug_output.setdefault("trace_data", []).append({
                            "x": pts.clone(), "d": distances,
                            "rays_alive": self.backend.get_rays(_backend.ALIVE),
                            "rays_hit": self.backend.get_rays(_backend.HIT)})
                    self.backend.advance_rays(distances)
                    i += 1
                with profile("sphere_tracer.compact_rays"):
                    n_rays_alive = self.backend.compact_rays()
                logger.debug("Trace step %d - %d (%.2f%%) rays alive", i, n_rays_alive, share(n_rays_alive))
        self.last_march_iters = i

        if self.tail_sample_threshold > 0 and n_rays_alive > 0:
            with profile("sphere_tracer.tail_sample"):
                rays_samples_offset, rays_n_samples, rays_sample_depths, rays_sample_positions \
                    = self.backend.sample_on_segments(self.tail_sample_step_size)
                rays_sample_distances = query_sdf(rays_sample_positions)
                self.backend.trace_on_samples(rays_samples_offset, rays_n_samples, rays_sample_depths, rays_sample_distances)
        return self.backend.get_rays(_backend.HIT)
