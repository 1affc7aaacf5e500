"""nr3d_lib_amd.bindings._sphere_trace -- drop-in for the reference pybind module ``nr3d_lib.bindings._sphere_trace``
(csrc/sphere_trace/src/entry.cu:14-47), backed by the HIP kernels of csrc/sphere_trace.hip through include/nr3d_hip.h.

Same Python-visible names, argument order / defaults and return structure:
  RayStatus (ALIVE, HIT, OUT exported), DenseGrid, SphereTracer, ray_march.

Deliberate differences ("Sphere tracer"):
  * ``advance_rays`` also writes the next query positions; ``get_trace_positions`` returns a VIEW of that buffer (no launch, no
    allocation), valid until the next ``advance_rays`` / ``compact_rays`` / ``init_rays``: clone it to keep it;
  * compaction is a stable scan: alive rays keep their order, hits are listed in the order they were compacted, run after run;
  * the state lives in torch tensors allocated once per ``init_rays``; counts reach the host through pinned words, one wait per
    compaction (and one per ``ray_march``, ``sample_on_segments``, ``trace_on_samples``);
  * ``DenseGrid`` keeps its grid tensor alive (the reference keeps a bare pointer);
  * no walk leaves a ray's own segments and a non-finite distance ends its ray as OUT (debug_flag -128);
  * ``n_steps`` is an int32 (the reference's uint16 wraps at 65536 steps);
  * ``segs_endpoint_distances`` and ``enable_debug=True`` are rejected (not ported); more argument checks, all before any launch.
"""
import enum

import torch

from .. import _hip as H

__all__ = ["RayStatus", "ALIVE", "HIT", "OUT", "DenseGrid", "SphereTracer", "ray_march"]


class RayStatus(enum.IntEnum):
    """sphere_tracer.cuh:8"""
    ALIVE = 0
    HIT = 1
    OUT = 2


ALIVE, HIT, OUT = RayStatus.ALIVE, RayStatus.HIT, RayStatus.OUT     # export_values() (entry.cu:15-19)


def _chk(fn, name, t, shape, dtype=torch.float32):
    """`t` is a contiguous CUDA tensor of `dtype` and `shape` (None in `shape`: any size)"""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{fn}: `{name}` must be a tensor, got {type(t).__name__}")
    H.require_gpu(t)
    if t.dtype != dtype:
        raise RuntimeError(f"{fn}: `{name}` must be {dtype}, got {t.dtype}")
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        want = "[" + ", ".join("n" if s is None else str(s) for s in shape) + "]"
        raise RuntimeError(f"{fn}: `{name}` must be {want}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{fn}: `{name}` must be contiguous")
    return t


def _same_device(fn, dev, **tensors):
    for name, t in tensors.items():
        if t.device != dev:
            raise RuntimeError(f"{fn}: `{name}` is on {t.device}, rays_o on {dev}")


class DenseGrid:
    """DenseGrid(x, y, z, grid_occ) (entry.cu:21-27): bool occupancy [x, y, z] over [-1, 1]^3"""

    def __init__(self, x: int, y: int, z: int, grid_occ: torch.Tensor):
        self._res = (int(x), int(y), int(z))
        if min(self._res) <= 0 or self._res[0] * self._res[1] * self._res[2] >= 2 ** 31:
            raise RuntimeError(f"DenseGrid: resolution {self._res} must be positive with fewer than 2^31 voxels")
        self.grid_occ = _chk("DenseGrid", "grid_occ", grid_occ, self._res, torch.bool)      # kept alive here

    @property
    def res(self):
        return self._res

    def _c_res(self):
        import ctypes as C
        return (C.c_int32 * 3)(*self._res)


def _rays(fn, rays_o, rays_d):
    _chk(fn, "rays_o", rays_o, (None, 3))
    _chk(fn, "rays_d", rays_d, (rays_o.shape[0], 3))
    _same_device(fn, rays_o.device, rays_d=rays_d)
    return rays_o.shape[0], rays_o.device


def _tmp(n, dev):
    return H.empty((int(H.lib().nr3d_sphere_trace_tmp_bytes(max(n, 1))) + 7) // 8, dtype=torch.int64, device=dev)


def ray_march(grid, rays_o, rays_d, rays_near, rays_far, return_pts=False, enable_debug=False):
    """-> (valid_rays_idx int64 [n_valid], segs_pack_info int32 [n_valid, 2], segs float [total, 2], segs_endpoints float
    [total, 2, 3] | None, {})  (ray_march.cu:64-129)"""
    fn = "ray_march"
    if enable_debug:
        raise RuntimeError("ray_march: enable_debug=True is not ported (the reference instantiates its non-debug kernel there too)")
    if not isinstance(grid, DenseGrid):
        raise RuntimeError(f"ray_march: `grid` must be a DenseGrid, got {type(grid).__name__}")
    n, dev = _rays(fn, rays_o, rays_d)
    _chk(fn, "rays_near", rays_near, (n,))
    _chk(fn, "rays_far", rays_far, (n,))
    _same_device(fn, dev, rays_near=rays_near, rays_far=rays_far, grid_occ=grid.grid_occ)
    if n >= 2 ** 28:
        raise RuntimeError(f"ray_march: {n} rays in one call, the limit is 2^28 - 1 (split the batch)")

    def out(n_valid, total):
        return (H.empty((n_valid, 2), dtype=torch.int32, device=dev), H.empty((total, 2), dtype=torch.float32, device=dev),
                H.empty((total, 2, 3), dtype=torch.float32, device=dev) if return_pts else None)

    if n == 0:
        return (torch.empty(0, dtype=torch.int64, device=dev),) + out(0, 0) + ({},)
    with H.on_device(dev):
        st, res = H.stream_of(rays_o), grid._c_res()
        valid = H.empty(n, dtype=torch.int64, device=dev)
        pack64 = H.empty((n, 2), dtype=torch.int64, device=dev)
        totals = H.host_i64(2, dev)
        tmp = _tmp(n, dev)
        H.check(H.lib().nr3d_sphere_trace_march_count(n, H.ptr(rays_o), H.ptr(rays_d), H.ptr(rays_near), H.ptr(rays_far), res,
                                                      H.ptr(grid.grid_occ), H.ptr(valid), H.ptr(pack64), H.ptr(totals), H.ptr(tmp), st))
        total, n_valid = H.wait_i64(totals, dev)            # the single device->host sync of this op
        if total >= 2 ** 31:
            raise RuntimeError(f"ray_march: {total} segments do not fit the int32 pack table (split the batch)")
        pack, segs, pts = out(n_valid, total)
        H.check(H.lib().nr3d_sphere_trace_march_write(n_valid, H.ptr(rays_o), H.ptr(rays_d), H.ptr(rays_near), H.ptr(rays_far), res,
                                                      H.ptr(grid.grid_occ), H.ptr(valid), H.ptr(pack64), total, H.ptr(pack),
                                                      H.ptr(segs), H.ptr(pts), st))
    return valid[:n_valid], pack, segs, pts, {}


class SphereTracer:
    """SphereTracer(min_step, distance_scale, zero_offset=0, hit_threshold=1e-3) (entry.cu:29-43, sphere_tracer.cuh:48-101)"""

    def __init__(self, min_step: float, distance_scale: float, zero_offset: float = 0.0, hit_threshold: float = 0.001):
        self._min_step, self._distance_scale = float(min_step), float(distance_scale)
        self._zero_offset, self._hit_threshold = float(zero_offset), float(hit_threshold)
        self._dev = None
        self._cap = self._n_total = self._n_alive = self._n_hit = self._buf = 0
        self._state = self._hits = self._tmp = self._rays_o = self._rays_d = self._segs = None

    # ---- state ------------------------------------------------------------------------------------------------------
    def init_rays(self, rays_o, rays_d, valid_rays_idx, segs_pack_info, segs, segs_endpoint_distances=None):
        """sphere_tracer.cu:416-453"""
        fn = "init_rays"
        if segs_endpoint_distances is not None:
            raise RuntimeError("init_rays: `segs_endpoint_distances` (the distance-hint variant) is not ported: the reference's Python "
                               "never passes it and its advance loop has no bound")
        n_rays, dev = _rays(fn, rays_o, rays_d)
        _chk(fn, "valid_rays_idx", valid_rays_idx, (None,), torch.int64)
        n = valid_rays_idx.shape[0]
        _chk(fn, "segs_pack_info", segs_pack_info, (n, 2), torch.int32)
        _chk(fn, "segs", segs, (None, 2))
        _same_device(fn, dev, valid_rays_idx=valid_rays_idx, segs_pack_info=segs_pack_info, segs=segs)
        if n_rays >= 2 ** 31 or n >= 2 ** 28:
            raise RuntimeError(f"init_rays: {n_rays} rays / {n} valid rays in one call (limits 2^31 - 1 / 2^28 - 1)")
        self._dev, self._rays_o, self._rays_d, self._segs = dev, rays_o, rays_d, segs
        self._cap = self._n_total = self._n_alive = n
        self._n_hit = self._buf = 0
        self._state = self._hits = self._tmp = None
        if n == 0:
            return
        with H.on_device(dev):
            l = H.lib()
            sb = int(l.nr3d_sphere_trace_state_bytes(n))
            self._state = [H.empty(sb, dtype=torch.uint8, device=dev) for _ in range(2)]
            self._hits = H.empty(int(l.nr3d_sphere_trace_hits_bytes(n)), dtype=torch.uint8, device=dev)
            self._tmp = _tmp(n, dev)
            H.check(l.nr3d_sphere_trace_init(n, n_rays, segs.shape[0], H.ptr(rays_o), H.ptr(rays_d), H.ptr(valid_rays_idx),
                                             H.ptr(segs_pack_info), H.ptr(segs), H.ptr(self._state[0]), n, H.stream_of(rays_o)))

    def _need_init(self, fn):
        if self._dev is None:
            raise RuntimeError(f"{fn}: call init_rays first")

    def compact_rays(self) -> int:
        """-> number of alive rays (sphere_tracer.cu:455-470); one host wait"""
        self._need_init("compact_rays")
        if self._n_alive == 0:
            return 0
        dev = self._dev
        with H.on_device(dev):
            totals = H.host_i64(2, dev)
            H.check(H.lib().nr3d_sphere_trace_compact(self._n_alive, H.ptr(self._state[self._buf]), H.ptr(self._state[1 - self._buf]),
                                                      self._cap, H.ptr(self._hits), self._n_hit, H.ptr(totals), H.ptr(self._tmp),
                                                      H.stream_of(self._rays_o)))
            n_alive, n_new = H.wait_i64(totals, dev)
        self._buf = 1 - self._buf
        self._n_alive, self._n_hit = n_alive, self._n_hit + n_new
        return n_alive

    def advance_rays(self, distances):
        """sphere_tracer.cu:472-487; also leaves the next query positions behind (get_trace_positions)"""
        fn = "advance_rays"
        self._need_init(fn)
        if not isinstance(distances, torch.Tensor) or distances.numel() != self._n_alive:
            raise RuntimeError(f"advance_rays: `distances` must hold one value per alive ray ({self._n_alive}), got "
                               f"{list(distances.shape) if isinstance(distances, torch.Tensor) else type(distances).__name__}")
        if self._n_alive == 0:
            return
        _chk(fn, "distances", distances, tuple(distances.shape))
        _same_device(fn, self._dev, distances=distances)
        with H.on_device(self._dev):
            H.check(H.lib().nr3d_sphere_trace_advance(self._n_alive, H.ptr(self._rays_o), H.ptr(self._rays_d), H.ptr(distances),
                                                      H.ptr(self._segs), H.ptr(self._state[self._buf]), self._cap, self._zero_offset,
                                                      self._distance_scale, self._min_step, self._hit_threshold,
                                                      H.stream_of(self._rays_o)))

    def n_rays(self, status) -> int:
        """sphere_tracer.cuh:76-80"""
        status = RayStatus(status)
        if status == OUT:
            return self._n_total - self._n_alive - self._n_hit
        return self._n_alive if status == ALIVE else self._n_hit

    def get_rays(self, status):
        """sphere_tracer.cu:489-547: dict of n_rays, pos, dir, idx, t, n_steps (+ status, debug_flag, hit_region_infos,
        hit_seg_regions, seg_idxs, seg_end_idxs for ALIVE)"""
        status = RayStatus(status)
        if status == OUT:
            raise ValueError("Cannot get rays of status OUT")
        self._need_init("get_rays")
        dev, n = self._dev, self.n_rays(status)
        e = lambda shape, dtype: H.empty(shape, dtype=dtype, device=dev)   # noqa: E731
        ret = {"n_rays": torch.scalar_tensor(n), "pos": e((n, 3), torch.float32), "dir": e((n, 3), torch.float32),
               "idx": e(n, torch.int64), "t": e(n, torch.float32), "n_steps": e(n, torch.int32)}
        if status == ALIVE:
            ret.update(status=e(n, torch.uint8), debug_flag=e(n, torch.int8), hit_region_infos=e((n, 4), torch.float32),
                       hit_seg_regions=e((n, 2), torch.int32), seg_idxs=e(n, torch.int32), seg_end_idxs=e(n, torch.int32))
        if n == 0:
            return ret
        common = (H.ptr(ret["pos"]), H.ptr(ret["dir"]), H.ptr(ret["idx"]), H.ptr(ret["t"]), H.ptr(ret["n_steps"]))
        with H.on_device(dev):
            st = H.stream_of(self._rays_o)
            if status == HIT:
                H.check(H.lib().nr3d_sphere_trace_gather_hit(n, H.ptr(self._rays_o), H.ptr(self._rays_d), H.ptr(self._hits), self._cap,
                                                             *common, st))
            else:
                H.check(H.lib().nr3d_sphere_trace_gather_alive(
                    n, H.ptr(self._rays_o), H.ptr(self._rays_d), H.ptr(self._state[self._buf]), self._cap, *common,
                    H.ptr(ret["status"]), H.ptr(ret["debug_flag"]), H.ptr(ret["hit_region_infos"]), H.ptr(ret["hit_seg_regions"]),
                    H.ptr(ret["seg_idxs"]), H.ptr(ret["seg_end_idxs"]), st))
        return ret

    def get_trace_positions(self):
        """query positions of the alive rays, float [n_alive, 3] (sphere_tracer.cu:549-559): a view of the buffer ``init_rays`` /
        ``advance_rays`` / ``compact_rays`` maintain -- no launch; overwritten by the next of those calls"""
        self._need_init("get_trace_positions")
        n = self._n_alive
        if n == 0:
            return torch.empty((0, 3), dtype=torch.float32, device=self._dev)
        off = 24 * ((self._cap + 3) // 4 * 4)                    # behind hit_region (16 B) and hit_seg (8 B) of csrc/sphere_trace.hip's State
        return self._state[self._buf][off:off + 12 * n].view(torch.float32).view(n, 3)

    # ---- tail sampling ------------------------------------------------------------------------------------------------
    def sample_on_segments(self, step_size: float):
        """-> (rays_samples_offset int32 [n_alive], rays_n_samples int32 [n_alive], rays_sample_depths float [total],
        rays_sample_positions float [total, 3])  (sphere_tracer.cu:561-593); one host wait"""
        self._need_init("sample_on_segments")
        step_size = float(step_size)
        if not step_size > 0.0:
            raise RuntimeError(f"sample_on_segments: `step_size` must be positive, got {step_size}")
        dev, n = self._dev, self._n_alive
        e = lambda shape, dtype: H.empty(shape, dtype=dtype, device=dev)   # noqa: E731
        if n == 0:
            return e(0, torch.int32), e(0, torch.int32), e(0, torch.float32), e((0, 3), torch.float32)
        with H.on_device(dev):
            l, st = H.lib(), H.stream_of(self._rays_o)
            pack = e((n, 2), torch.int32)
            total_w = H.host_i64(1, dev)
            H.check(l.nr3d_sphere_trace_sample_count(n, step_size, H.ptr(self._segs), H.ptr(self._state[self._buf]), self._cap,
                                                     H.ptr(pack), H.ptr(total_w), H.ptr(self._tmp), st))
            total = H.wait_i64(total_w, dev)[0]
            if total >= 2 ** 31:
                raise RuntimeError(f"sample_on_segments: {total} samples do not fit int32 offsets (use a larger step_size)")
            offs, cnts = e(n, torch.int32), e(n, torch.int32)
            depths, pos = e(total, torch.float32), e((total, 3), torch.float32)
            H.check(l.nr3d_sphere_trace_sample_write(n, step_size, H.ptr(self._rays_o), H.ptr(self._rays_d), H.ptr(self._segs),
                                                     H.ptr(self._state[self._buf]), self._cap, H.ptr(pack), total, H.ptr(offs),
                                                     H.ptr(cnts), H.ptr(depths), H.ptr(pos), st))
        return offs, cnts, depths, pos

    def trace_on_samples(self, rays_samples_offset, rays_n_samples, rays_sample_depths, rays_sample_distances):
        """the first sign change of every alive ray's samples becomes a hit (sphere_tracer.cu:595-604); one host wait"""
        fn = "trace_on_samples"
        self._need_init(fn)
        n, dev = self._n_alive, self._dev
        _chk(fn, "rays_samples_offset", rays_samples_offset, (n,), torch.int32)
        _chk(fn, "rays_n_samples", rays_n_samples, (n,), torch.int32)
        _chk(fn, "rays_sample_depths", rays_sample_depths, (None,))
        total = rays_sample_depths.shape[0]
        if not isinstance(rays_sample_distances, torch.Tensor) or rays_sample_distances.numel() != total:
            raise RuntimeError(f"trace_on_samples: `rays_sample_distances` must hold one value per sample ({total})")
        _chk(fn, "rays_sample_distances", rays_sample_distances, tuple(rays_sample_distances.shape))
        _same_device(fn, dev, rays_samples_offset=rays_samples_offset, rays_n_samples=rays_n_samples,
                     rays_sample_depths=rays_sample_depths, rays_sample_distances=rays_sample_distances)
        if n == 0:
            return
        if self._n_hit + n > self._cap:
            raise RuntimeError("trace_on_samples: the hit list is full (called twice on the same alive rays?)")
        with H.on_device(dev):
            totals = H.host_i64(2, dev)
            H.check(H.lib().nr3d_sphere_trace_trace_on_samples(
                n, H.ptr(self._state[self._buf]), self._cap, H.ptr(rays_samples_offset), H.ptr(rays_n_samples), total,
                H.ptr(rays_sample_depths), H.ptr(rays_sample_distances), H.ptr(self._hits), self._n_hit, H.ptr(totals), H.ptr(self._tmp),
                H.stream_of(self._rays_o)))
            self._n_hit += H.wait_i64(totals, dev)[1]

    # ---- the loop -----------------------------------------------------------------------------------------------------
    def trace(self, rays_o, rays_d, distance_function, max_steps_between_compact, max_march_iters, valid_rays_idx, segs_pack_info,
              segs, segs_endpoint_distances=None):
        """sphere_tracer.cu:606-620"""
        self.init_rays(rays_o, rays_d, valid_rays_idx, segs_pack_info, segs, segs_endpoint_distances)
        i = 1
        while i < max_march_iters and self._n_alive > 0:
            for _ in range(min(i, max_steps_between_compact)):
                self.advance_rays(distance_function(self.get_trace_positions()))
                i += 1
            self.compact_rays()
