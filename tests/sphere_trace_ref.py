"""numpy float32 restatement of the sphere tracer's device code -- the checker of nr3d_lib_amd/csrc/sphere_trace.hip.

Restates the reference's csrc/sphere_trace (file:line cited at every piece) one operation per rounding, in the kernels' order, vectorised
over the rays (every ray makes exactly the scalar code's decisions; the lock-step loops only let rays that are done wait).  nvcc is absent,
so the reference itself cannot produce fixtures; tests/test_sphere_trace_cpu.py pins this file with answers worked out by hand.

Conventions shared with the kernels (csrc/sphere_trace.hip's header comment):
  * an FMA exactly where nvcc's default contraction makes one: ``fma32`` below, evaluated EXACTLY (one rounding), not as two operations;
  * float -> int by truncation, made total (``f2i``): NaN / beyond +-2^30 becomes a voxel far outside the grid;
  * the DDA is one loop over two phases with the cap rx + ry + rz + 2;
  * the segment walks of advance_single_step stay inside the ray's own [first, end) segments, a non-finite distance ends the ray as OUT;
  * both sampling phases clamp a segment's sample count at 0;
  * compaction is stable: alive rays keep their order, hits are appended in buffer order.
"""
import numpy as np

F = np.float32
ALIVE, HIT, OUT = 0, 1, 2
KFAR = -(1 << 30)


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, correctly rounded: the product of two float32 is exact in float64 (48 bits), the sum is
    rounded to ODD in float64 (TwoSum gives the rounding error's sign), and a round-to-odd value with 53 >= 2 * 24 + 2 bits rounds to
    the float32 the exact sum rounds to."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    shape = a.shape
    a64, b64, c64 = (v.astype(np.float64).reshape(-1) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a64 * b64
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F).reshape(shape)


def f2i(f):
    """(int)f as glm::ivec3(vec3) does (truncation), total: csrc/sphere_trace.hip f2i"""
    f = np.asarray(f, F)
    with np.errstate(all="ignore"):
        ok = np.abs(f) < F(1073741824.0)
        return np.where(ok, np.trunc(np.where(ok, f, F(0))).astype(np.int32), np.int32(KFAR))


def _voxel_idx(voxel, res):
    """dense_grid.cuh:18-24"""
    rx, ry, rz = res
    x, y, z = (voxel[:, i].astype(np.int64) for i in range(3))
    inside = (x >= 0) & (x < rx) & (y >= 0) & (y < ry) & (z >= 0) & (z < rz)
    return np.where(inside, x * ry * rz + y * rz + z, -1)


def ray_march(grid_occ, rays_o, rays_d, rays_near, rays_far, return_pts=False):
    """dense_grid.cuh:38-67 (advance_to_next_voxel), :117-200 (ray_march), ray_march.cu:11-129 ->
    (valid_rays_idx int64 [nv], segs_pack_info int32 [nv, 2], segs float32 [T, 2], endpoints float32 [T, 2, 3] | None)"""
    occ = np.ascontiguousarray(grid_occ, dtype=bool)
    res = occ.shape
    flat = occ.reshape(-1)
    o, d = np.asarray(rays_o, F).reshape(-1, 3), np.asarray(rays_d, F).reshape(-1, 3)
    near, far = np.asarray(rays_near, F).reshape(-1), np.asarray(rays_far, F).reshape(-1)
    n = o.shape[0]
    ar = np.arange(n)
    with np.errstate(all="ignore"):
        sc = F(0.5) * np.array(res, dtype=F)                         # ray_march.cu:24
        origin = (o + F(1.0)) * sc                                   # :25
        dr = d * sc                                                  # :26
        inv_dir = F(1.0) / (dr + F(1e-10))                           # dense_grid.cuh:128
        sgn = 1 - np.signbit(dr).astype(np.int32)                    # :129-130
        a = np.abs(dr)
        k = np.where((a[:, 0] > a[:, 1]) & (a[:, 0] > a[:, 2]), 0, np.where((a[:, 1] > a[:, 0]) & (a[:, 1] > a[:, 2]), 1, 2))   # :132-134
        inv_k, origin_k = inv_dir[ar, k], origin[ar, k]
        pos = fma32(dr, near[:, None], origin)                       # :136 (contracted)
        voxel = f2i(pos)                                             # :137
        vidx = _voxel_idx(voxel, res)
        occ0 = (vidx >= 0) & flat[np.maximum(vidx, 0)]
        t_enter = np.where(occ0, (pos[ar, k] - origin_k) * inv_k, F(0)).astype(F)      # :159 when no walk came first
        active = ~(occ0 & ~(t_enter < far))                          # :161
        run = occ0 & active
        ev_ray, ev_t0, ev_t1 = [], [], []
        cap = res[0] + res[1] + res[2] + 2
        for _ in range(cap):
            ix = np.nonzero(active)[0]
            if ix.size == 0:
                break
            r = np.arange(ix.size)
            p, v, dd, sg = pos[ix], voxel[ix], dr[ix], sgn[ix]
            ng = v + sg                                              # dense_grid.cuh:43
            txyz = (ng.astype(F) - p) * inv_dir[ix]                  # :44
            axis = np.where(txyz[:, 0] < txyz[:, 1], 0, 1)           # :47
            axis = np.where(txyz[r, axis] < txyz[:, 2], axis, 2)     # :48
            ta = txyz[r, axis]
            newp = fma32(ta[:, None], dd, p)                         # :58-59 (contracted)
            newp[r, axis] = ng[r, axis].astype(F)                    # :57
            v[r, axis] += sg[r, axis] * 2 - 1                        # :54
            pos[ix], voxel[ix] = newp, v
            vi = _voxel_idx(v, res)
            oc = (vi >= 0) & flat[np.maximum(vi, 0)]
            tk = ((newp[r, k[ix]] - origin_k[ix]) * inv_k[ix]).astype(F)
            rn, fr = run[ix], far[ix]
            # GAP phase (dense_grid.cuh:145-158, 184-197): leaves at an occupied voxel or outside the grid
            gap_end = ~rn & ~((vi >= 0) & ~oc)
            enter = gap_end & (vi >= 0) & (tk < fr)                  # :161
            # RUN phase (:162-183)
            run_end = rn & ~oc
            stop = run_end & ((vi < 0) | (tk >= fr))                 # :182
            if run_end.any():
                ev_ray.append(ix[run_end])
                ev_t0.append(t_enter[ix[run_end]])
                ev_t1.append(np.fmin(tk[run_end], fr[run_end]))      # :177
            t_enter[ix[enter]] = tk[enter]
            run[ix[enter]] = True
            run[ix[run_end]] = False
            active[ix[(gap_end & ~enter) | stop]] = False
    if ev_ray:
        ray, t0, t1 = np.concatenate(ev_ray), np.concatenate(ev_t0), np.concatenate(ev_t1)
        order = np.argsort(ray, kind="stable")                       # a ray's events are already in march order
        ray, t0, t1 = ray[order], t0[order], t1[order]
    else:
        ray, t0, t1 = np.zeros(0, np.int64), np.zeros(0, F), np.zeros(0, F)
    counts = np.bincount(ray, minlength=n).astype(np.int64)
    valid = np.nonzero(counts)[0].astype(np.int64)                   # ray_march.cu:100
    cnt = counts[valid]
    pack = np.stack([np.cumsum(cnt) - cnt, cnt], -1).astype(np.int32).reshape(-1, 2)      # :105-107
    segs = np.stack([t0, t1], -1).astype(F).reshape(-1, 2)
    pts = None
    if return_pts:                                                   # :50-53 (contracted)
        pts = np.stack([fma32(d[ray], t0[:, None], o[ray]), fma32(d[ray], t1[:, None], o[ray])], 1).astype(F).reshape(-1, 2, 3)
    return valid, pack, segs, pts


class SphereTracer:
    """sphere_tracer.cu: the tracer state as arrays and its steps"""

    def __init__(self, min_step, distance_scale, zero_offset=0.0, hit_threshold=1e-3):
        self.min_step, self.distance_scale = F(min_step), F(distance_scale)
        self.zero_offset, self.hit_threshold = F(zero_offset), F(hit_threshold)

    def init_rays(self, rays_o, rays_d, valid_rays_idx, segs_pack_info, segs):
        """sphere_tracer.cu:93-121"""
        self.o, self.d = np.asarray(rays_o, F).reshape(-1, 3), np.asarray(rays_d, F).reshape(-1, 3)
        self.segs = np.asarray(segs, F).reshape(-1, 2)
        valid = np.asarray(valid_rays_idx, np.int64).reshape(-1)
        pack = np.asarray(segs_pack_info, np.int32).reshape(-1, 2)
        n = valid.shape[0]
        first, cnt = pack[:, 0].astype(np.int64), pack[:, 1].astype(np.int64)
        ok = (valid >= 0) & (valid < self.o.shape[0]) & (first >= 0) & (cnt > 0) & (first + cnt <= self.segs.shape[0])
        end = np.where(ok, first + cnt, 0)
        first = np.where(ok, first, 0)
        self.n_total = n
        self.idx = np.where(ok, valid, 0).astype(np.int32)
        self.seg_idx, self.seg_first, self.seg_end = first.astype(np.int32), first.astype(np.int32), end.astype(np.int32)
        self.n_steps = np.zeros(n, np.int32)
        self.status = np.where(ok, ALIVE, OUT).astype(np.uint8)
        self.dbg = np.zeros(n, np.int8)
        sg = self.segs if self.segs.shape[0] else np.zeros((1, 2), F)
        self.t = np.where(ok, sg[first, 0], F(0)).astype(F)
        self.hr = np.stack([np.full(n, -1, F), np.where(ok, sg[np.maximum(end - 1, 0), 1], F(0)).astype(F), np.full(n, -1, F),
                            np.full(n, 1, F)], -1).reshape(-1, 4)
        self.hs = np.stack([first, end], -1).astype(np.int32).reshape(-1, 2)
        self.hits = [np.zeros(0, np.int32), np.zeros(0, F), np.zeros(0, np.int32)]

    @property
    def n_alive(self):
        return self.idx.shape[0]

    def positions(self):
        """sphere_tracer.cu:248-262 (contracted)"""
        return fma32(self.d[self.idx], self.t[:, None], self.o[self.idx]).reshape(-1, 3)

    def advance_rays(self, distances):
        """sphere_tracer.cu:212-246 with :36-91 (one pass of its loop: no endpoint distances) and :11-34"""
        dist = np.asarray(distances, F).reshape(-1)
        assert dist.shape[0] == self.n_alive
        if self.n_alive == 0:
            return
        t, hr, hs, seg_idx, segs = self.t, self.hr, self.hs, self.seg_idx, self.segs
        with np.errstate(all="ignore"):
            alive = self.status == ALIVE                              # :226
            d = fma32(dist, self.distance_scale, -self.zero_offset)  # :231 (contracted)
            fin = np.isfinite(d)
            bad = alive & ~fin
            self.status[bad], self.dbg[bad] = OUT, -128
            m = alive & fin
            c1 = m & ((hr[:, 2] < 0) | (d >= 0))                      # :48-56
            c2 = m & ~c1
            hr[c1, 0], hr[c1, 2], hs[c1, 0] = t[c1], d[c1], seg_idx[c1]
            hr[c2, 1], hr[c2, 3], hs[c2, 1] = t[c2], d[c2], seg_idx[c2] + 1
            h1 = m & (np.abs(d) <= self.hit_threshold)                # :61-65
            t[h1] = t[h1] + d[h1]
            self.dbg[h1], self.status[h1] = 127, HIT
            rest = m & ~h1
            width = hr[:, 1] - hr[:, 0]
            h2 = rest & (hr[:, 2] >= 0) & (hr[:, 3] <= 0) & (width <= F(1.1) * self.min_step)    # :66-73
            kk = hr[:, 2] / (hr[:, 2] - hr[:, 3])
            t[h2] = fma32(kk, width, hr[:, 0])[h2]
            self.dbg[h2], self.status[h2] = 126, HIT
            mv = rest & ~h2
            fw = mv & (~np.signbit(d) | (hr[:, 2] < 0))               # :77
            bw = mv & ~fw
            ad = np.abs(d)
            seg = segs[seg_idx]
            # forward (:15-26); the walk stops at the ray's last segment
            t[fw] = (t + np.fmax(np.fmin(ad, width * F(0.8)), self.min_step))[fw]
            while True:
                go = fw & (t > seg[:, 1]) & (seg_idx + 1 < self.seg_end)
                if not go.any():
                    break
                seg_idx[go] += 1
                seg = segs[seg_idx]
            ok = fw & (t <= seg[:, 1])
            t[ok] = np.fmax(t, seg[:, 0])[ok]
            out = fw & ~ok
            t[out] = seg[out, 1]
            self.status[out] = OUT
            # backward (:27-33); the walk stops at the ray's first segment
            t[bw] = (t - np.fmin(width / F(2.0), np.fmax(ad, self.min_step)))[bw]
            while True:
                go = bw & (t < seg[:, 0]) & (seg_idx > self.seg_first)
                if not go.any():
                    break
                seg_idx[go] -= 1
                seg = segs[seg_idx]
            t[bw] = np.fmin(t, seg[:, 1])[bw]
            self.n_steps[mv] += 1                                     # :80
            self.dbg[mv] = np.where(out, -127, np.where(fw, 1, -1))[mv]      # :81

    def compact_rays(self):
        """sphere_tracer.cu:177-210, 455-470, with a stable order instead of atomicAdd tickets"""
        h = self.status == HIT
        self.hits = [np.concatenate([self.hits[0], self.idx[h]]), np.concatenate([self.hits[1], self.t[h]]),
                     np.concatenate([self.hits[2], self.n_steps[h]])]
        a = self.status == ALIVE
        for name in ("idx", "seg_idx", "seg_first", "seg_end", "n_steps", "status", "dbg", "t", "hr", "hs"):
            setattr(self, name, getattr(self, name)[a].copy())
        return self.n_alive

    def n_rays(self, status):
        n_hit = self.hits[0].shape[0]
        return self.n_alive if status == ALIVE else n_hit if status == HIT else self.n_total - self.n_alive - n_hit

    def get_rays(self, status):
        """sphere_tracer.cu:264-323, 489-547"""
        if status == HIT:
            idx, t, steps = self.hits
            return dict(pos=fma32(self.d[idx], t[:, None], self.o[idx]).reshape(-1, 3), dir=self.d[idx].reshape(-1, 3),
                        idx=idx.astype(np.int64), t=t, n_steps=steps)
        return dict(pos=self.positions(), dir=self.d[self.idx].reshape(-1, 3), idx=self.idx.astype(np.int64), t=self.t, n_steps=self.n_steps,
                    status=self.status, debug_flag=self.dbg, hit_region_infos=self.hr, hit_seg_regions=self.hs, seg_idxs=self.seg_idx,
                    seg_end_idxs=self.seg_end)

    def _seg_samples(self, si, i, step):
        """sphere_tracer.cu:336-339, 361-366 -> (count, start, length)"""
        with np.errstate(all="ignore"):
            x0 = np.fmax(self.segs[si, 0], self.hr[i, 0])
            ln = F(np.fmin(self.segs[si, 1], self.hr[i, 1]) - x0)
            c = int(f2i(np.ceil(ln / step)))
        return (0 if c == KFAR else max(0, c + 1)), F(x0), ln

    def sample_on_segments(self, step_size):
        """sphere_tracer.cu:325-373, 561-593 -> (offsets int32, counts int32, depths, positions)"""
        step = F(step_size)
        counts, depths, owner = [], [], []
        for i in range(self.n_alive):
            lo, hi = max(int(self.hs[i, 0]), int(self.seg_first[i])), min(int(self.hs[i, 1]), int(self.seg_end[i]))
            c = 0
            for si in range(lo, hi):
                m, x0, ln = self._seg_samples(si, i, step)
                with np.errstate(all="ignore"):
                    ds = F(ln / F(m - 1))                             # :366
                ts = x0
                for _ in range(m):
                    depths.append(ts)
                    with np.errstate(all="ignore"):
                        ts = F(ts + ds)                               # :368
                c += m
            counts.append(c)
            owner += [int(self.idx[i])] * c
        counts = np.array(counts, np.int64).reshape(-1)
        depths, owner = np.array(depths, F).reshape(-1), np.array(owner, np.int64).reshape(-1)
        pos = fma32(self.d[owner], depths[:, None], self.o[owner]).reshape(-1, 3)         # :370 (contracted)
        return (np.cumsum(counts) - counts).astype(np.int32), counts.astype(np.int32), depths, pos

    def trace_on_samples(self, offsets, counts, depths, distances):
        """sphere_tracer.cu:375-399, hits appended in buffer order"""
        depths, dist = np.asarray(depths, F).reshape(-1), np.asarray(distances, F).reshape(-1)
        hi, ht, hn = [], [], []
        for i in range(self.n_alive):
            off, cnt = int(offsets[i]), int(counts[i])
            for p in range(off, off + cnt - 1):
                d1, d2 = dist[p], dist[p + 1]
                if d1 >= 0 and d2 <= 0:
                    with np.errstate(all="ignore"):
                        k = F(d1 / F(d1 - d2))
                    ht.append(fma32(k, F(depths[p + 1] - depths[p]), depths[p]).reshape(()))          # :393 (contracted)
                    hi.append(self.idx[i])
                    hn.append(self.n_steps[i] + cnt)
                    break
        self.hits = [np.concatenate([self.hits[0], np.array(hi, np.int32).reshape(-1)]),
                     np.concatenate([self.hits[1], np.array(ht, F).reshape(-1)]),
                     np.concatenate([self.hits[2], np.array(hn, np.int32).reshape(-1)])]

    def trace(self, rays_o, rays_d, distance_function, max_steps_between_compact, max_march_iters, valid_rays_idx, segs_pack_info, segs):
        """sphere_tracer.cu:606-620"""
        self.init_rays(rays_o, rays_d, valid_rays_idx, segs_pack_info, segs)
        i = 1
        while i < max_march_iters and self.n_alive > 0:
            for _ in range(min(i, max_steps_between_compact)):
                self.advance_rays(distance_function(self.positions()))
                i += 1
            self.compact_rays()


# ---- the scene both test files trace ----------------------------------------------------------------------------------------------
def sphere_scene(res=32, n_side=24):
    """a camera at (0, 0, -0.95) inside the grid looking at a sphere of radius 0.5; occupancy: every voxel within a voxel diagonal of
    the ball"""
    c = (np.arange(res, dtype=np.float64) + 0.5) / res * 2 - 1
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    grid = np.sqrt(X * X + Y * Y + Z * Z) < 0.5 + 2 * np.sqrt(3) / res
    u = np.linspace(-0.7, 0.7, n_side)
    U, V = np.meshgrid(u, u, indexing="ij")
    d = np.stack([U.ravel(), V.ravel(), np.ones(U.size)], -1)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    o = np.tile(np.array([0, 0, -0.95], F), (d.shape[0], 1))
    return grid, o, d, np.zeros(d.shape[0], F), np.full(d.shape[0], 3, F)


def sphere_sdf(x, radius=0.5):
    return (np.sqrt((x.astype(np.float64) ** 2).sum(-1)) - radius).astype(F)


def analytic_sphere_hits(o, d, radius, margin):
    """rays whose line passes within radius - margin of the origin (hit) / beyond radius + margin (miss); the rest graze"""
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    tc = -(o64 * d64).sum(-1)
    dist = np.linalg.norm(o64 + tc[:, None] * d64, axis=1)
    return (dist < radius - margin) & (tc > 0), dist > radius + margin
