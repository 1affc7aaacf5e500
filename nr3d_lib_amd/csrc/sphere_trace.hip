// nr3d_lib_amd/csrc/sphere_trace.hip -- dense-grid segment march and the sphere tracer's state and steps (gfx950).
// Restates the reference's csrc/sphere_trace (dense_grid.cuh, ray_march.cu, sphere_tracer.cu); C ABI: include/nr3d_hip.h
// (nr3d_sphere_trace_*), Python twin: nr3d_lib_amd/bindings/_sphere_trace.py, numpy restatement: tests/sphere_trace_ref.py.
//
// What differs from a transliteration ("Sphere tracer"):
//   * one tracer launch per step: k_advance writes the next query positions itself (it holds o, d and the new t);
//   * compaction is a stable scan (scan.h): alive rays keep their order, hits are appended in payload order; no global atomics;
//   * the state is a structure of arrays inside ONE caller-provided block per buffer side (State below), nothing is allocated
//     here, the alive / hit totals go to caller-provided words (pinned host memory in the bindings);
//   * every loop has a bound and every index a guard, whatever the distances (see dda_cap, advance_single_step, k_init).
//
// Floating point: the library builds with -ffp-contract=off.  The explicit fmaf() below are exactly the places where nvcc's default
// (--fmad=true) contracts the reference's expressions:
//   pos = origin + dir * near                     (dense_grid.cuh:136)       fmaf(dir, near, origin)
//   new_pos[a1] = pos[a1] + txyz[axis] * dir[a1]  (dense_grid.cuh:58-59)     fmaf(txyz[axis], dir[a1], pos[a1])
//   endpoint = origin + dir * seg.{x,y}           (ray_march.cu:51-52)       fmaf(dir, seg, origin)
//   d = distances[i] * distance_scale - zero_off  (sphere_tracer.cu:231)     fmaf(dist, scale, -zero_offset)
//   t = x + k * (y - x)                           (sphere_tracer.cu:70,393)  fmaf(k, y - x, x)
//   position = ray_o + ray_d * t                  (sphere_tracer.cu:261,289,318,370)  fmaf(ray_d, t, ray_o)
// Everything else (the (x + 1) * scale of the grid transform, (next_grid - pos) * inv_dir, (pos - origin) * inv_k, 0.8f * region,
// 1.1f * min_step, ...) is a product of a sum or a lone product and stays as separate roundings.
#include "common.h"
#include "scan.h"
#include "compact.h"

namespace nr3d {
namespace st {

constexpr int kBlock = 256;
enum : uint8_t { ALIVE = 0, HIT = 1, OUT = 2 };     // sphere_tracer.cuh:8

// float -> int as the reference's glm::ivec3(vec3) (truncation), made total: the reference's conversion is undefined for NaN and
// beyond int range; here such a coordinate becomes a voxel far outside any grid (its ray then gets no segment).
constexpr int32_t kFar = -(1 << 30);
__device__ __forceinline__ int32_t f2i(float f) { return fabsf(f) < 1073741824.0f ? (int32_t)f : kFar; }

__device__ __forceinline__ float get3(const float3 &v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }
__device__ __forceinline__ int32_t get3(const int3 &v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }

struct Grid {
	int32_t rx, ry, rz;
	const uint8_t *occ;        // bool [rx, ry, rz]
	// dense_grid.cuh:18-24
	__device__ __forceinline__ int32_t voxel_idx(const int3 &v) const {
		if (v.x < 0 || v.x >= rx || v.y < 0 || v.y >= ry || v.z < 0 || v.z >= rz) return -1;
		return v.x * ry * rz + v.y * rz + v.z;
	}
	// The DDA moves one voxel per step in a fixed direction per axis (dir_sign never changes), so a walk that is inside the grid
	// leaves it within rx + ry + rz steps; a start outside takes one step first and a last step leaves: rx + ry + rz + 2.  The
	// walk below is ONE loop with this explicit cap on top of the argument (NaN directions still step an axis by +-1).
	__device__ __forceinline__ int32_t dda_cap() const { return rx + ry + rz + 2; }
};

// dense_grid.cuh:38-67 advance_to_next_voxel
__device__ __forceinline__ void dda_step(float3 &pos, int3 &voxel, const float3 &dir, const float3 &inv_dir, const int3 &sgn) {
	const int3 ng = make_int3(voxel.x + sgn.x, voxel.y + sgn.y, voxel.z + sgn.z);
	const float3 txyz = make_float3(((float)ng.x - pos.x) * inv_dir.x, ((float)ng.y - pos.y) * inv_dir.y, ((float)ng.z - pos.z) * inv_dir.z);
	int axis = txyz.x < txyz.y ? 0 : 1;                // first minimum
	axis = get3(txyz, axis) < txyz.z ? axis : 2;
	const float ta = get3(txyz, axis);
	pos = make_float3(axis == 0 ? (float)ng.x : fmaf(ta, dir.x, pos.x), axis == 1 ? (float)ng.y : fmaf(ta, dir.y, pos.y),
	                  axis == 2 ? (float)ng.z : fmaf(ta, dir.z, pos.z));
	if (axis == 0) voxel.x += sgn.x * 2 - 1; else if (axis == 1) voxel.y += sgn.y * 2 - 1; else voxel.z += sgn.z * 2 - 1;
}

// dense_grid.cuh:117-200 ray_march, as one bounded loop over two phases (GAP: looking for an occupied voxel, RUN: inside a run).
// o / d: the ray in world space (grid over [-1, 1]^3).  WRITE: at most max_segs segments are written (the count of phase 1).
template <bool WRITE>
__device__ __forceinline__ int32_t march(const Grid &g, const float3 &o, const float3 &d, float near, float far, int32_t max_segs,
                                         float2 *__restrict__ segs, float *__restrict__ endpoints) {
	// ray_march.cu:24-26: space_scale = 0.5 * res, origin = (o + 1) * scale, dir = d * scale
	const float3 sc = make_float3(0.5f * (float)g.rx, 0.5f * (float)g.ry, 0.5f * (float)g.rz);
	const float3 origin = make_float3((o.x + 1.0f) * sc.x, (o.y + 1.0f) * sc.y, (o.z + 1.0f) * sc.z);
	const float3 dir = make_float3(d.x * sc.x, d.y * sc.y, d.z * sc.z);
	const float3 inv_dir = make_float3(1.0f / (dir.x + 1e-10f), 1.0f / (dir.y + 1e-10f), 1.0f / (dir.z + 1e-10f));
	// dir_sign = 1 - signbit (dense_grid.cuh:129-130), the sign BIT: -0.0f counts as negative
	const int3 sgn = make_int3(1 - (int)(__float_as_uint(dir.x) >> 31), 1 - (int)(__float_as_uint(dir.y) >> 31), 1 - (int)(__float_as_uint(dir.z) >> 31));
	const float ax = fabsf(dir.x), ay = fabsf(dir.y), az = fabsf(dir.z);
	const int k = (ax > ay && ax > az) ? 0 : ((ay > ax && ay > az) ? 1 : 2);      // strict >: ties go to z
	const float inv_k = get3(inv_dir, k), origin_k = get3(origin, k);
	float3 pos = make_float3(fmaf(dir.x, near, origin.x), fmaf(dir.y, near, origin.y), fmaf(dir.z, near, origin.z));
	int3 voxel = make_int3(f2i(pos.x), f2i(pos.y), f2i(pos.z));
	int32_t vidx = g.voxel_idx(voxel);
	int32_t n_segs = 0;
	float t_enter = 0.0f;
	bool run = false;
	if (vidx >= 0 && g.occ[vidx]) {       // starts inside an occupied voxel: no walk before the first segment
		t_enter = (get3(pos, k) - origin_k) * inv_k;
		if (!(t_enter < far)) return 0;
		run = true;
	}
	const int32_t cap = g.dda_cap();
	for (int32_t it = 0; it < cap; ++it) {
		dda_step(pos, voxel, dir, inv_dir, sgn);
		vidx = g.voxel_idx(voxel);
		const bool occ = vidx >= 0 && g.occ[vidx];
		if (!run) {
			if (vidx >= 0 && !occ) continue;
			t_enter = (get3(pos, k) - origin_k) * inv_k;
			if (!(vidx >= 0 && t_enter < far)) break;
			run = true;
		} else {
			if (occ) continue;
			const float t_exit = (get3(pos, k) - origin_k) * inv_k;
			if (WRITE) {
				if (n_segs >= max_segs) break;
				const float t1 = fminf(t_exit, far);
				segs[n_segs] = make_float2(t_enter, t1);
				if (endpoints) {
					float *e = endpoints + 6 * (size_t)n_segs;
					e[0] = fmaf(d.x, t_enter, o.x); e[1] = fmaf(d.y, t_enter, o.y); e[2] = fmaf(d.z, t_enter, o.z);
					e[3] = fmaf(d.x, t1, o.x); e[4] = fmaf(d.y, t1, o.y); e[5] = fmaf(d.z, t1, o.z);
				}
			}
			++n_segs;
			if (vidx < 0 || t_exit >= far) break;
			run = false;
		}
	}
	return n_segs;
}

__device__ __forceinline__ float3 ld3(const float *__restrict__ p, size_t i) { return make_float3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
__device__ __forceinline__ void st3(float *__restrict__ p, size_t i, const float3 &v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }
__device__ __forceinline__ float3 along(const float3 &o, const float3 &d, float t) {
	return make_float3(fmaf(d.x, t, o.x), fmaf(d.y, t, o.y), fmaf(d.z, t, o.z));
}

// ray_march.cu:11-32
__global__ __launch_bounds__(kBlock) void k_march_count(uint32_t n, Grid g, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                        const float *__restrict__ near, const float *__restrict__ far,
                                                        int32_t *__restrict__ counts) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	counts[i] = march<false>(g, ld3(rays_o, i), ld3(rays_d, i), near[i], far[i], 0, nullptr, nullptr);
}

// ray_march.cu:34-62; also narrows the scan's int64 (begin, count) rows to the reference's int32 pack table
__global__ __launch_bounds__(kBlock) void k_march_write(uint32_t n_valid, Grid g, const float *__restrict__ rays_o,
                                                        const float *__restrict__ rays_d, const float *__restrict__ near,
                                                        const float *__restrict__ far, const int64_t *__restrict__ valid_idx,
                                                        const int64_t *__restrict__ pack64, int64_t total_segs,
                                                        int32_t *__restrict__ pack32, float2 *__restrict__ segs,
                                                        float *__restrict__ endpoints) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n_valid) return;
	const int64_t r = valid_idx[i], begin = pack64[2 * i], cnt = pack64[2 * i + 1];
	pack32[2 * i] = (int32_t)begin;
	pack32[2 * i + 1] = (int32_t)cnt;
	if (begin < 0 || cnt < 0 || begin + cnt > total_segs) return;         // never outside the caller's buffers
	march<true>(g, ld3(rays_o, r), ld3(rays_d, r), near[r], far[r], (int32_t)cnt, segs + begin, endpoints ? endpoints + 6 * begin : nullptr);
}

// ------------------------------------------------------------------------------------------------
// tracer state: structure of arrays inside one block of state_bytes(cap) bytes (sphere_tracer.cuh:10-44 TracePayload /
// TraceBuffer as arrays; `seg_first` and `pos` are additions: the ray's first segment bounds the backward walk, `pos` is the
// next query position the step kernel leaves behind)
// ------------------------------------------------------------------------------------------------
struct State {
	float4 *hit_region;     // t0, t1, d0, d1
	int2 *hit_seg;
	float *pos;             // [cap, 3]
	float *t;
	int32_t *idx, *seg_idx, *seg_end, *seg_first, *n_steps;
	uint8_t *status;
	int8_t *dbg;
};
static __host__ __device__ inline uint64_t cap4(uint32_t cap) { return ((uint64_t)cap + 3ull) & ~3ull; }
static __host__ __device__ inline uint64_t state_bytes(uint32_t cap) { return cap4(cap) * 62ull; }
static __host__ __device__ inline State view(void *base, uint32_t cap) {
	const uint64_t c = cap4(cap);
	char *p = (char *)base;
	State s;
	s.hit_region = (float4 *)p; p += 16 * c;
	s.hit_seg = (int2 *)p; p += 8 * c;
	s.pos = (float *)p; p += 12 * c;
	s.t = (float *)p; p += 4 * c;
	s.idx = (int32_t *)p; p += 4 * c;
	s.seg_idx = (int32_t *)p; p += 4 * c;
	s.seg_end = (int32_t *)p; p += 4 * c;
	s.seg_first = (int32_t *)p; p += 4 * c;
	s.n_steps = (int32_t *)p; p += 4 * c;
	s.status = (uint8_t *)p; p += c;
	s.dbg = (int8_t *)p;
	return s;
}
// hit list (sphere_tracer.cuh:19-23 HitPayload as arrays): hits_bytes(cap) bytes
struct Hits { int32_t *idx; float *t; int32_t *n_steps; };
static __host__ __device__ inline uint64_t hits_bytes(uint32_t cap) { return cap4(cap) * 12ull; }
static __host__ __device__ inline Hits hview(void *base, uint32_t cap) {
	const uint64_t c = cap4(cap);
	Hits h;
	h.idx = (int32_t *)base; h.t = (float *)((char *)base + 4 * c); h.n_steps = (int32_t *)((char *)base + 8 * c);
	return h;
}

// sphere_tracer.cu:93-121 init_rays_kernel.  A row the kernels could not follow safely (ray index outside [0, n_rays), an empty pack
// or one outside [0, n_segs)) starts as OUT instead of being trusted.
__global__ __launch_bounds__(kBlock) void k_init(uint32_t n, uint32_t n_rays, int64_t n_segs, const float *__restrict__ rays_o,
                                                 const float *__restrict__ rays_d, const int64_t *__restrict__ valid_idx,
                                                 const int32_t *__restrict__ pack, const float2 *__restrict__ segs, State s) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	const int64_t r = valid_idx[i];
	const int32_t first = pack[2 * i], cnt = pack[2 * i + 1];
	const bool ok = r >= 0 && r < (int64_t)n_rays && first >= 0 && cnt > 0 && (int64_t)first + cnt <= n_segs;
	const int32_t end = ok ? first + cnt : 0;
	const float t = ok ? segs[first].x : 0.0f;
	s.idx[i] = ok ? (int32_t)r : 0;
	s.seg_idx[i] = ok ? first : 0;
	s.seg_first[i] = ok ? first : 0;
	s.seg_end[i] = end;
	s.n_steps[i] = 0;
	s.status[i] = ok ? ALIVE : OUT;
	s.dbg[i] = 0;
	s.t[i] = t;
	s.hit_region[i] = make_float4(-1.0f, ok ? segs[end - 1].y : 0.0f, -1.0f, 1.0f);
	s.hit_seg[i] = make_int2(ok ? first : 0, end);
	st3(s.pos, i, ok ? along(ld3(rays_o, r), ld3(rays_d, r), t) : make_float3(0.0f, 0.0f, 0.0f));
}

// sphere_tracer.cu:11-34 advance_single_step.  Both walks stay inside the ray's own segments [first, end): the reference's forward
// walk tests `seg_idx < seg_end_idx` before `++seg_idx` and so reads segs[seg_end_idx], the NEXT ray's first segment (or past the
// buffer for the last ray), and its backward walk has no lower bound at all.  Here the forward walk stops at the ray's last segment
// (t beyond it: OUT at that segment's end, which is what the reference's comment says it means) and the backward walk at its first.
__device__ __forceinline__ uint8_t advance_single_step(const float2 *__restrict__ segs, float min_step, float d, bool forward,
                                                       int32_t first, int32_t end, int32_t &seg_idx, const float4 &hr, float &t,
                                                       float2 &seg) {
	if (forward) {
		t += fmaxf(fminf(d, (hr.y - hr.x) * 0.8f), min_step);
		while (t > seg.y && seg_idx + 1 < end) seg = segs[++seg_idx];       // at most end - first iterations
		if (t <= seg.y) {
			t = fmaxf(t, seg.x);
			return ALIVE;
		}
		t = seg.y;
		return OUT;
	}
	t -= fminf((hr.y - hr.x) / 2.0f, fmaxf(d, min_step));
	while (t < seg.x && seg_idx > first) seg = segs[--seg_idx];             // at most end - first iterations
	t = fminf(t, seg.y);
	return ALIVE;
}

// sphere_tracer.cu:212-246 advance_rays_kernel + :36-91 advance_ray (without segs_endpoint_distances the reference's loop body runs
// once) + :248-262 get_positions_kernel for the NEXT step.  A non-finite distance ends the ray as OUT (debug_flag -128) before it
// touches the state.
__global__ __launch_bounds__(kBlock) void k_advance(uint32_t n, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                    const float *__restrict__ distances, const float2 *__restrict__ segs, State s,
                                                    float zero_offset, float distance_scale, float min_step, float hit_threshold) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	if (s.status[i] != ALIVE) return;          // compaction does not follow every step (sphere_tracer.cu:224-227); pos[i] is still o + d * t
	const float d = fmaf(distances[i], distance_scale, -zero_offset);
	if (!isfinite(d)) {
		s.status[i] = OUT;
		s.dbg[i] = -128;
		return;
	}
	float t = s.t[i];
	float4 hr = s.hit_region[i];
	int2 hs = s.hit_seg[i];
	int32_t seg_idx = s.seg_idx[i];
	const int32_t first = s.seg_first[i], end = s.seg_end[i];
	float2 seg = segs[seg_idx];
	uint8_t status;
	int8_t dbg;
	int32_t steps = s.n_steps[i];
	// a valid hit region starts outside: while its start is still inside (d0 < 0) the start moves along (sphere_tracer.cu:44-56)
	if (hr.z < 0.0f || d >= 0.0f) { hr.x = t; hr.z = d; hs.x = seg_idx; }
	else { hr.y = t; hr.w = d; hs.y = seg_idx + 1; }
	if (fabsf(d) <= hit_threshold) {
		t = t + d;
		dbg = 127;
		status = HIT;
	} else if (hr.z >= 0.0f && hr.w <= 0.0f && hr.y - hr.x <= 1.1f * min_step) {
		const float k = hr.z / (hr.z - hr.w);
		t = fmaf(k, hr.y - hr.x, hr.x);
		dbg = 126;
		status = HIT;
	} else {
		const bool forward = !(__float_as_uint(d) >> 31) || hr.z < 0.0f;
		status = advance_single_step(segs, min_step, fabsf(d), forward, first, end, seg_idx, hr, t, seg);
		++steps;
		dbg = status == OUT ? -127 : (forward ? 1 : -1);
	}
	s.t[i] = t;
	s.hit_region[i] = hr;
	s.hit_seg[i] = hs;
	s.seg_idx[i] = seg_idx;
	s.n_steps[i] = steps;
	s.status[i] = status;
	s.dbg[i] = dbg;
	const size_t r = (size_t)s.idx[i];
	st3(s.pos, i, along(ld3(rays_o, r), ld3(rays_d, r), t));
}

// ------------------------------------------------------------------------------------------------
// stable compaction (replaces sphere_tracer.cu:177-210's atomicAdd tickets): value(i) = (status == ALIVE) | (status == HIT) << 36,
// one exclusive scan gives a ray's rank among the alive rays (low bits) and among the new hits (high bits).  The scan of the tile
// sums and the totals store are compact.h's k_c_scan_tiles (totals[0] = alive, totals[1] = new hits, system scope).
// `Src` says where a row's hit payload comes from; MOVE: alive rows are copied to the other buffer side.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t sval(uint8_t status) {
	return status == ALIVE ? 1ull : (status == HIT ? (1ull << glue::kShift) : 0ull);
}

__global__ __launch_bounds__(scan::kThreads) void k_status_tile_sums(uint32_t n, const uint8_t *__restrict__ status,
                                                                     uint64_t *__restrict__ tile_sums) {
	__shared__ uint64_t lds[4];
	const uint64_t first = (uint64_t)blockIdx.x * scan::kTile + (uint64_t)threadIdx.x * scan::kItems;
	uint64_t v = 0;
#pragma unroll
	for (int k = 0; k < scan::kItems; ++k)
		if (first + k < n) v += sval(status[first + k]);
	uint64_t tot;
	scan::block_exclusive(v, tot, lds);
	if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

// SINGLE: n <= scan::kTile, one workgroup does the whole compaction in one launch and stores the totals itself
template <bool SINGLE, bool MOVE>
__global__ __launch_bounds__(scan::kThreads) void k_status_write(uint32_t n, const uint8_t *__restrict__ status,
                                                                 const int32_t *__restrict__ h_idx, const float *__restrict__ h_t,
                                                                 const int32_t *__restrict__ h_steps,
                                                                 const uint64_t *__restrict__ tile_prefix, State in, State out,
                                                                 Hits hits, uint32_t n_hit, uint32_t cap,
                                                                 int64_t *__restrict__ totals) {
	__shared__ uint64_t lds[4];
	const uint64_t first = (uint64_t)blockIdx.x * scan::kTile + (uint64_t)threadIdx.x * scan::kItems;
	uint64_t v[scan::kItems], sum = 0;
#pragma unroll
	for (int k = 0; k < scan::kItems; ++k) {
		v[k] = (first + k < n) ? sval(status[first + k]) : 0;
		sum += v[k];
	}
	uint64_t tot;
	uint64_t run = (SINGLE ? 0ull : tile_prefix[blockIdx.x]) + scan::block_exclusive(sum, tot, lds);
#pragma unroll
	for (int k = 0; k < scan::kItems; ++k) {
		const uint64_t i = first + k;
		if (i < n && v[k]) {
			if (v[k] == 1ull) {
				if (MOVE) {
					const uint64_t j = run & glue::kLow;
					out.hit_region[j] = in.hit_region[i];
					out.hit_seg[j] = in.hit_seg[i];
					out.pos[3 * j] = in.pos[3 * i]; out.pos[3 * j + 1] = in.pos[3 * i + 1]; out.pos[3 * j + 2] = in.pos[3 * i + 2];
					out.t[j] = in.t[i];
					out.idx[j] = in.idx[i];
					out.seg_idx[j] = in.seg_idx[i];
					out.seg_end[j] = in.seg_end[i];
					out.seg_first[j] = in.seg_first[i];
					out.n_steps[j] = in.n_steps[i];
					out.status[j] = ALIVE;
					out.dbg[j] = in.dbg[i];
				}
			} else {
				const uint64_t j = (uint64_t)n_hit + (run >> glue::kShift);
				if (j < cap) {                  // the hit list holds `cap` rows; the bindings refuse a call that could need more
					hits.idx[j] = h_idx[i];
					hits.t[j] = h_t[i];
					hits.n_steps[j] = h_steps[i];
				}
			}
		}
		run += v[k];
	}
	if (SINGLE && threadIdx.x == 0) {
		__hip_atomic_store(&totals[0], (int64_t)(tot & glue::kLow), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		__hip_atomic_store(&totals[1], (int64_t)(tot >> glue::kShift), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	}
}

template <bool MOVE>
static int compact(uint32_t n, const uint8_t *status, const int32_t *h_idx, const float *h_t, const int32_t *h_steps, State in, State out,
                   Hits hits, uint32_t n_hit, uint32_t cap, int64_t *totals, void *tmp, hipStream_t st) {
	if (n <= (uint32_t)scan::kTile) {
		hipLaunchKernelGGL((k_status_write<true, MOVE>), dim3(1), dim3(scan::kThreads), 0, st, n, status, h_idx, h_t, h_steps,
		                   (const uint64_t *)nullptr, in, out, hits, n_hit, cap, totals);
		NR3D_LAUNCH_CHECK();
		return 0;
	}
	const uint32_t n_tiles = div_up(n, scan::kTile);
	uint64_t *tile_sums = (uint64_t *)tmp;
	hipLaunchKernelGGL(k_status_tile_sums, dim3(n_tiles), dim3(scan::kThreads), 0, st, n, status, tile_sums);
	hipLaunchKernelGGL(glue::k_c_scan_tiles, dim3(1), dim3(scan::kThreads), 0, st, n_tiles, tile_sums, totals);
	hipLaunchKernelGGL((k_status_write<false, MOVE>), dim3(n_tiles), dim3(scan::kThreads), 0, st, n, status, h_idx, h_t, h_steps,
	                   (const uint64_t *)tile_sums, in, out, hits, n_hit, cap, totals);
	NR3D_LAUNCH_CHECK();
	return 0;
}

// sphere_tracer.cu:302-323 get_hit_rays_kernel
__global__ __launch_bounds__(kBlock) void k_gather_hit(uint32_t n, const float *__restrict__ rays_o, const float *__restrict__ rays_d, Hits h,
                                                       float *__restrict__ pos, float *__restrict__ dir, int64_t *__restrict__ idx,
                                                       float *__restrict__ t_out, int32_t *__restrict__ n_steps) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	const size_t r = (size_t)h.idx[i];
	const float t = h.t[i];
	const float3 d = ld3(rays_d, r);
	st3(pos, i, along(ld3(rays_o, r), d, t));
	st3(dir, i, d);
	idx[i] = (int64_t)r;
	t_out[i] = t;
	n_steps[i] = h.n_steps[i];
}

// sphere_tracer.cu:264-300 get_rays_kernel
__global__ __launch_bounds__(kBlock) void k_gather_alive(uint32_t n, const float *__restrict__ rays_o, const float *__restrict__ rays_d, State s,
                                                         float *__restrict__ pos, float *__restrict__ dir, int64_t *__restrict__ idx,
                                                         float *__restrict__ t_out, int32_t *__restrict__ n_steps,
                                                         uint8_t *__restrict__ status, int8_t *__restrict__ dbg,
                                                         float4 *__restrict__ hit_region, int2 *__restrict__ hit_seg,
                                                         int32_t *__restrict__ seg_idx, int32_t *__restrict__ seg_end) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	const size_t r = (size_t)s.idx[i];
	const float t = s.t[i];
	const float3 d = ld3(rays_d, r);
	st3(pos, i, along(ld3(rays_o, r), d, t));
	st3(dir, i, d);
	idx[i] = (int64_t)r;
	t_out[i] = t;
	n_steps[i] = s.n_steps[i];
	status[i] = s.status[i];
	dbg[i] = s.dbg[i];
	hit_region[i] = s.hit_region[i];
	hit_seg[i] = s.hit_seg[i];
	seg_idx[i] = s.seg_idx[i];
	seg_end[i] = s.seg_end[i];
}

// samples of one segment clipped to the hit region (sphere_tracer.cu:336-339, 361-366).  Both phases use the write phase's
// max(0, .) -- the reference's count phase omits it, so a clipped-away segment there SUBTRACTS from the ray's count and the two phases
// disagree.  The float -> int conversion is total (f2i).
__device__ __forceinline__ int32_t seg_samples(float2 seg, float t0, float t1, float step, float &x0, float &len) {
	x0 = fmaxf(seg.x, t0);
	len = fminf(seg.y, t1) - x0;
	const int32_t c = f2i(ceilf(len / step));
	return c == kFar ? 0 : max(0, c + 1);
}

// sphere_tracer.cu:325-342 sample_on_segments_phase1_kernel; the segment range is clamped to the ray's own [first, end)
__global__ __launch_bounds__(kBlock) void k_sample_count(uint32_t n, float step, const float2 *__restrict__ segs, State s,
                                                         int32_t *__restrict__ counts) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	const float4 hr = s.hit_region[i];
	const int2 hs = s.hit_seg[i];
	const int32_t lo = max(hs.x, s.seg_first[i]), hi = min(hs.y, s.seg_end[i]);
	int64_t c = 0;
	for (int32_t si = lo; si < hi; ++si) {
		float x0, len;
		c += seg_samples(segs[si], hr.x, hr.y, step, x0, len);
	}
	counts[i] = c < 0x7fffffffll ? (int32_t)c : 0x7fffffff;
}

// sphere_tracer.cu:344-373 sample_on_segments_phase2_kernel; never writes more than the ray's counted samples
__global__ __launch_bounds__(kBlock) void k_sample_write(uint32_t n, float step, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                         const float2 *__restrict__ segs, State s, const int32_t *__restrict__ pack,
                                                         int64_t total, int32_t *__restrict__ offsets, int32_t *__restrict__ counts,
                                                         float *__restrict__ depths, float *__restrict__ positions) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	const int32_t off = pack[2 * i], cnt = pack[2 * i + 1];
	offsets[i] = off;
	counts[i] = cnt;
	if (off < 0 || cnt < 0 || (int64_t)off + cnt > total) return;
	const size_t r = (size_t)s.idx[i];
	const float3 o = ld3(rays_o, r), d = ld3(rays_d, r);
	const float4 hr = s.hit_region[i];
	const int2 hs = s.hit_seg[i];
	const int32_t lo = max(hs.x, s.seg_first[i]), hi = min(hs.y, s.seg_end[i]);
	int32_t w = 0;
	for (int32_t si = lo; si < hi; ++si) {
		float x0, len;
		const int32_t m = seg_samples(segs[si], hr.x, hr.y, step, x0, len);
		const float ds = len / (float)(m - 1);
		float ts = x0;
		for (int32_t j = 0; j < m && w < cnt; ++j, ++w, ts += ds) {
			depths[off + w] = ts;
			st3(positions, (size_t)off + w, along(o, d, ts));
		}
	}
}

// sphere_tracer.cu:375-399 trace_on_samples_kernel, first half: the first bracket of every ray -> a hit payload in scratch; the
// stable append (compact<false>) replaces its atomicAdd ticket
__global__ __launch_bounds__(kBlock) void k_trace_samples(uint32_t n, State s, const int32_t *__restrict__ offsets,
                                                          const int32_t *__restrict__ counts, int64_t total,
                                                          const float *__restrict__ depths, const float *__restrict__ dist,
                                                          uint8_t *__restrict__ flag, float *__restrict__ h_t, int32_t *__restrict__ h_steps) {
	const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
	if (i >= n) return;
	const int32_t off = offsets[i], cnt = counts[i];
	uint8_t f = OUT;
	float t = 0.0f;
	if (off >= 0 && cnt >= 0 && (int64_t)off + cnt <= total) {
		for (int32_t p = off; p < off + cnt - 1; ++p) {
			const float d1 = dist[p], d2 = dist[p + 1];
			if (d1 >= 0.0f && d2 <= 0.0f) {
				const float t1 = depths[p], t2 = depths[p + 1];
				const float k = d1 / (d1 - d2);
				t = fmaf(k, t2 - t1, t1);
				f = HIT;
				break;
			}
		}
	}
	flag[i] = f;
	h_t[i] = t;
	h_steps[i] = s.n_steps[i] + cnt;
}

static inline uint64_t tmp_bytes(uint32_t n) { return cap4(n) * 16ull + scan::tmp_bytes(n); }

}  // namespace st
}  // namespace nr3d

using namespace nr3d;

static int st_grid(const int32_t res[3], const uint8_t *occ, st::Grid &g) {
	NR3D_CHECK(res && occ, "sphere_trace: NULL grid pointer");
	NR3D_CHECK(res[0] > 0 && res[1] > 0 && res[2] > 0 && (int64_t)res[0] * res[1] * res[2] < (1ll << 31),
	           "sphere_trace: grid resolution (%d, %d, %d) must be positive with fewer than 2^31 voxels", res[0], res[1], res[2]);
	g = st::Grid{res[0], res[1], res[2], occ};
	return 0;
}

extern "C" uint64_t nr3d_sphere_trace_state_bytes(uint32_t cap) { return st::state_bytes(cap); }
extern "C" uint64_t nr3d_sphere_trace_hits_bytes(uint32_t cap) { return st::hits_bytes(cap); }
extern "C" uint64_t nr3d_sphere_trace_tmp_bytes(uint32_t n) { return st::tmp_bytes(n); }

extern "C" int nr3d_sphere_trace_march_count(uint32_t n_rays, const float *rays_o, const float *rays_d, const float *rays_near,
                                             const float *rays_far, const int32_t grid_res[3], const uint8_t *grid_occ,
                                             int64_t *valid_rays_idx, int64_t *pack_infos, int64_t *totals, void *tmp, void *stream) {
	hipStream_t s = (hipStream_t)stream;
	NR3D_CHECK(totals, "sphere_trace_march_count: NULL totals");
	if (n_rays == 0) { NR3D_HIP_CHECK(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s)); return 0; }
	NR3D_CHECK(rays_o && rays_d && rays_near && rays_far && valid_rays_idx && pack_infos && tmp, "sphere_trace_march_count: NULL tensor pointer");
	st::Grid g;
	if (st_grid(grid_res, grid_occ, g)) return 1;
	int32_t *counts = (int32_t *)tmp;
	void *tiles = (char *)tmp + st::cap4(n_rays) * 16ull;
	hipLaunchKernelGGL(st::k_march_count, dim3(div_up(n_rays, st::kBlock)), dim3(st::kBlock), 0, s, n_rays, g, rays_o, rays_d, rays_near,
	                   rays_far, counts);
	NR3D_LAUNCH_CHECK();
	glue::PackWriter<int32_t, 1> w{counts, nullptr, nullptr, valid_rays_idx, pack_infos};
	return glue::compact_packs<int32_t, 1>(n_rays, w, totals, tiles, s);
}

extern "C" int nr3d_sphere_trace_march_write(uint32_t n_valid, const float *rays_o, const float *rays_d, const float *rays_near,
                                             const float *rays_far, const int32_t grid_res[3], const uint8_t *grid_occ,
                                             const int64_t *valid_rays_idx, const int64_t *pack_infos, int64_t total_segs,
                                             int32_t *segs_pack_info, float *segs, float *segs_endpoints, void *stream) {
	if (n_valid == 0) return 0;
	NR3D_CHECK(rays_o && rays_d && rays_near && rays_far && valid_rays_idx && pack_infos && segs_pack_info && segs,
	           "sphere_trace_march_write: NULL tensor pointer");
	NR3D_CHECK(total_segs >= 0 && total_segs <= 0x7fffffffll, "sphere_trace_march_write: %lld segments do not fit the int32 pack table",
	           (long long)total_segs);
	st::Grid g;
	if (st_grid(grid_res, grid_occ, g)) return 1;
	hipLaunchKernelGGL(st::k_march_write, dim3(div_up(n_valid, st::kBlock)), dim3(st::kBlock), 0, (hipStream_t)stream, n_valid, g, rays_o,
	                   rays_d, rays_near, rays_far, valid_rays_idx, pack_infos, total_segs, segs_pack_info, (float2 *)segs, segs_endpoints);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_sphere_trace_init(uint32_t n, uint32_t n_rays, int64_t n_segs, const float *rays_o, const float *rays_d,
                                      const int64_t *valid_rays_idx, const int32_t *segs_pack_info, const float *segs, void *state,
                                      uint32_t cap, void *stream) {
	if (n == 0) return 0;
	NR3D_CHECK(n <= cap, "sphere_trace_init: %u rays, state capacity %u", n, cap);
	NR3D_CHECK(rays_o && rays_d && valid_rays_idx && segs_pack_info && segs && state, "sphere_trace_init: NULL tensor pointer");
	hipLaunchKernelGGL(st::k_init, dim3(div_up(n, st::kBlock)), dim3(st::kBlock), 0, (hipStream_t)stream, n, n_rays, n_segs, rays_o, rays_d,
	                   valid_rays_idx, segs_pack_info, (const float2 *)segs, st::view(state, cap));
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_sphere_trace_advance(uint32_t n, const float *rays_o, const float *rays_d, const float *distances, const float *segs,
                                         void *state, uint32_t cap, float zero_offset, float distance_scale, float min_step,
                                         float hit_threshold, void *stream) {
	if (n == 0) return 0;
	NR3D_CHECK(n <= cap, "sphere_trace_advance: %u rays, state capacity %u", n, cap);
	NR3D_CHECK(rays_o && rays_d && distances && segs && state, "sphere_trace_advance: NULL tensor pointer");
	hipLaunchKernelGGL(st::k_advance, dim3(div_up(n, st::kBlock)), dim3(st::kBlock), 0, (hipStream_t)stream, n, rays_o, rays_d, distances,
	                   (const float2 *)segs, st::view(state, cap), zero_offset, distance_scale, min_step, hit_threshold);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_sphere_trace_compact(uint32_t n, void *state_in, void *state_out, uint32_t cap, void *hits, uint32_t n_hit,
                                         int64_t *totals, void *tmp, void *stream) {
	hipStream_t s = (hipStream_t)stream;
	NR3D_CHECK(totals, "sphere_trace_compact: NULL totals");
	if (n == 0) { NR3D_HIP_CHECK(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s)); return 0; }
	NR3D_CHECK(n <= cap && n_hit <= cap, "sphere_trace_compact: %u rays and %u hits, capacity %u", n, n_hit, cap);
	NR3D_CHECK(state_in && state_out && state_in != state_out && hits && tmp, "sphere_trace_compact: NULL or aliased buffer");
	const st::State in = st::view(state_in, cap);
	return st::compact<true>(n, in.status, in.idx, in.t, in.n_steps, in, st::view(state_out, cap), st::hview(hits, cap), n_hit, cap, totals,
	                         tmp, s);
}

extern "C" int nr3d_sphere_trace_gather_hit(uint32_t n_hit, const float *rays_o, const float *rays_d, const void *hits, uint32_t cap,
                                            float *pos, float *dir, int64_t *idx, float *t, int32_t *n_steps, void *stream) {
	if (n_hit == 0) return 0;
	NR3D_CHECK(n_hit <= cap, "sphere_trace_gather_hit: %u hits, capacity %u", n_hit, cap);
	NR3D_CHECK(rays_o && rays_d && hits && pos && dir && idx && t && n_steps, "sphere_trace_gather_hit: NULL tensor pointer");
	hipLaunchKernelGGL(st::k_gather_hit, dim3(div_up(n_hit, st::kBlock)), dim3(st::kBlock), 0, (hipStream_t)stream, n_hit, rays_o, rays_d,
	                   st::hview((void *)hits, cap), pos, dir, idx, t, n_steps);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_sphere_trace_gather_alive(uint32_t n, const float *rays_o, const float *rays_d, const void *state, uint32_t cap,
                                              float *pos, float *dir, int64_t *idx, float *t, int32_t *n_steps, uint8_t *status,
                                              int8_t *debug_flag, float *hit_region_infos, int32_t *hit_seg_regions, int32_t *seg_idxs,
                                              int32_t *seg_end_idxs, void *stream) {
	if (n == 0) return 0;
	NR3D_CHECK(n <= cap, "sphere_trace_gather_alive: %u rays, capacity %u", n, cap);
	NR3D_CHECK(rays_o && rays_d && state && pos && dir && idx && t && n_steps && status && debug_flag && hit_region_infos &&
	           hit_seg_regions && seg_idxs && seg_end_idxs, "sphere_trace_gather_alive: NULL tensor pointer");
	hipLaunchKernelGGL(st::k_gather_alive, dim3(div_up(n, st::kBlock)), dim3(st::kBlock), 0, (hipStream_t)stream, n, rays_o, rays_d,
	                   st::view((void *)state, cap), pos, dir, idx, t, n_steps, status, debug_flag, (float4 *)hit_region_infos,
	                   (int2 *)hit_seg_regions, seg_idxs, seg_end_idxs);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_sphere_trace_sample_count(uint32_t n, float step_size, const float *segs, const void *state, uint32_t cap,
                                              int32_t *pack_info, int64_t *total, void *tmp, void *stream) {
	hipStream_t s = (hipStream_t)stream;
	NR3D_CHECK(total, "sphere_trace_sample_count: NULL total");
	if (n == 0) { NR3D_HIP_CHECK(hipMemsetAsync(total, 0, sizeof(int64_t), s)); return 0; }
	NR3D_CHECK(n <= cap, "sphere_trace_sample_count: %u rays, capacity %u", n, cap);
	NR3D_CHECK(step_size > 0.0f, "sphere_trace_sample_count: step_size must be positive");
	NR3D_CHECK(segs && state && pack_info && tmp, "sphere_trace_sample_count: NULL tensor pointer");
	int32_t *counts = (int32_t *)tmp;
	void *tiles = (char *)tmp + st::cap4(n) * 16ull;
	hipLaunchKernelGGL(st::k_sample_count, dim3(div_up(n, st::kBlock)), dim3(st::kBlock), 0, s, n, step_size, (const float2 *)segs,
	                   st::view((void *)state, cap), counts);
	NR3D_LAUNCH_CHECK();
	return scan::pack_infos_from_counts<int32_t, int32_t>(n, counts, pack_info, total, tiles, s);
}

extern "C" int nr3d_sphere_trace_sample_write(uint32_t n, float step_size, const float *rays_o, const float *rays_d, const float *segs,
                                              const void *state, uint32_t cap, const int32_t *pack_info, int64_t total,
                                              int32_t *samples_offset, int32_t *n_samples, float *sample_depths,
                                              float *sample_positions, void *stream) {
	if (n == 0) return 0;
	NR3D_CHECK(n <= cap, "sphere_trace_sample_write: %u rays, capacity %u", n, cap);
	NR3D_CHECK(step_size > 0.0f && total >= 0 && total <= 0x7fffffffll, "sphere_trace_sample_write: step_size must be positive and the "
	           "samples (%lld) fit int32 offsets", (long long)total);
	NR3D_CHECK(rays_o && rays_d && segs && state && pack_info && samples_offset && n_samples && (total == 0 || (sample_depths && sample_positions)),
	           "sphere_trace_sample_write: NULL tensor pointer");
	hipLaunchKernelGGL(st::k_sample_write, dim3(div_up(n, st::kBlock)), dim3(st::kBlock), 0, (hipStream_t)stream, n, step_size, rays_o, rays_d,
	                   (const float2 *)segs, st::view((void *)state, cap), pack_info, total, samples_offset, n_samples, sample_depths,
	                   sample_positions);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_sphere_trace_trace_on_samples(uint32_t n, const void *state, uint32_t cap, const int32_t *samples_offset,
                                                  const int32_t *n_samples, int64_t total, const float *sample_depths,
                                                  const float *sample_distances, void *hits, uint32_t n_hit, int64_t *totals, void *tmp,
                                                  void *stream) {
	hipStream_t s = (hipStream_t)stream;
	NR3D_CHECK(totals, "sphere_trace_trace_on_samples: NULL totals");
	if (n == 0) { NR3D_HIP_CHECK(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s)); return 0; }
	NR3D_CHECK(n <= cap && (uint64_t)n_hit + n <= cap, "sphere_trace_trace_on_samples: %u rays and %u hits do not fit the hit list (%u)", n,
	           n_hit, cap);
	NR3D_CHECK(state && samples_offset && n_samples && hits && tmp && (total == 0 || (sample_depths && sample_distances)),
	           "sphere_trace_trace_on_samples: NULL tensor pointer");
	const uint64_t c = st::cap4(n);
	float *h_t = (float *)tmp;
	int32_t *h_steps = (int32_t *)((char *)tmp + 4 * c);
	uint8_t *flag = (uint8_t *)((char *)tmp + 8 * c);
	void *tiles = (char *)tmp + 16 * c;
	const st::State in = st::view((void *)state, cap);
	hipLaunchKernelGGL(st::k_trace_samples, dim3(div_up(n, st::kBlock)), dim3(st::kBlock), 0, s, n, in, samples_offset, n_samples, total,
	                   sample_depths, sample_distances, flag, h_t, h_steps);
	NR3D_LAUNCH_CHECK();
	return st::compact<false>(n, flag, in.idx, h_t, h_steps, in, in, st::hview(hits, cap), n_hit, cap, totals, tiles, s);
}
