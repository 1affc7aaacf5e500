// nr3d_lib_amd/csrc/nerfpp_march.hip -- the NeRF++ distant-view shell marcher (nr3d_nerfpp_march_count / _emit): the samples of every ray
// on N concentric shells around the close-range box (cuboid, ellipsoid, cubic or spherical shells; radii spaced in 1 / r or in log10 r),
// written once, packed, in (ray, shell) order.
//
// The reference runs this as a chain of torch ops (NeRFRendererMixinDistant._ray_marching, nr3d_lib/models/fields_distant/nerf/
// renderer_mixin.py:170-288): dense [R, N (+ 1)] tensors of radii, every ray against every shell, diff / addcmul / cat / norm, then
// nonzero(), four fancy-index gathers and a second nonzero() over the packs.  A sample depends on a handful of per-ray numbers and the
// table of N radii only, so here it is recomputed in registers: one wave per ray, lane = shell in chunks of 64, four rays per workgroup.
// A lane intersects the ray with its own shell AND with the next one (the delta): the kernels are bound by their stores, the second
// intersection is a few dozen VALU instructions, and nothing crosses lanes but the ballot.  No LDS, no atomics, no scratch.
//   count: ballot + popcount per chunk -> counts[ray];
//   (host: nr3d_prune_compact_packs turns counts into begin_all, the hit rays, their pack_infos and the totals -- one readback)
//   emit:  position = begin_all[ray] + valid shells of the chunks before + valid lanes below; x is one 16-byte store per lane.
// Both kernels call shell_sample(), compiled without contraction or fast math (Makefile), so they agree on every validity bit.
//
// All arithmetic is float32 in the chain's order of operations (the table in include/nr3d_hip.h); min / max over the slabs PROPAGATE NaN
// as torch.minimum / maximum / max(dim) / min(dim) do, where fminf / fmaxf would drop it.
#include "common.h"

namespace nr3d {
namespace nerfpp {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

// what a wave knows about its ray (wave-uniform)
struct Ray {
	float o[3], d[3];        // the ray the shells are intersected with: normalised (BOX, ELLIPSOID) or object space (CUBE, SPHERICAL)
	float c[3], h[3];        // the box: centre, half-extent
	float scale;             // shell radius -> intersection radius: 1 (BOX, ELLIPSOID), min_k stretch_k (CUBE, SPHERICAL)
	float pp, vv, pv;        // o.o, d.d, o.d
	float t_min;
};

__device__ __forceinline__ float nan_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a < b ? a : b)); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

__device__ __forceinline__ Ray load_ray(uint32_t ray, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                        const float *__restrict__ t_min, const float *__restrict__ aabb, int sample_mode) {
	Ray q;
	float stretch[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const float lo = aabb[k], hi = aabb[3 + k];
		q.c[k] = (hi + lo) / 2.0f;
		q.h[k] = (hi - lo) / 2.0f;
		stretch[k] = hi - lo;
	}
	const bool normalised = sample_mode == NR3D_NERFPP_BOX || sample_mode == NR3D_NERFPP_ELLIPSOID;
	q.scale = normalised ? 1.0f : nan_min(nan_min(stretch[0], stretch[1]), stretch[2]);
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const float o = rays_o[3 * (size_t)ray + k], d = rays_d[3 * (size_t)ray + k];
		q.o[k] = normalised ? (o - q.c[k]) / q.h[k] : o;
		q.d[k] = normalised ? d / q.h[k] : d;
	}
	q.pp = q.o[0] * q.o[0] + q.o[1] * q.o[1] + q.o[2] * q.o[2];
	q.vv = q.d[0] * q.d[0] + q.d[1] * q.d[1] + q.d[2] * q.d[2];
	q.pv = q.o[0] * q.d[0] + q.o[1] * q.d[1] + q.o[2] * q.d[2];
	q.t_min = t_min[ray];
	return q;
}

// ray_box_intersect (:53-82): the far crossing of the box of half side r, NaN where the ray misses it or it lies behind the origin
__device__ __forceinline__ float box_t(const Ray &q, float r) {
	float t_near = 0.0f, t_far = 0.0f;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const float a = (-r - q.o[k]) / q.d[k];
		const float b = (r - q.o[k]) / q.d[k];
		const float lo = nan_min(a, b), hi = nan_max(a, b);
		t_near = k == 0 ? lo : nan_max(t_near, lo);
		t_far = k == 0 ? hi : nan_min(t_far, hi);
	}
	return ((t_far > t_near) && (t_far > 0.0f)) ? t_far : __builtin_nanf("");
}

// ray_sphere_intersect (:31-50)
__device__ __forceinline__ float sphere_t(const Ray &q, float r) {
	return (sqrtf(q.pv * q.pv - q.vv * (q.pp - r * r)) - q.pv) / q.vv;
}

__device__ __forceinline__ float shell_t(const Ray &q, int sample_mode, float r) {
	const float rr = (sample_mode == NR3D_NERFPP_CUBE || sample_mode == NR3D_NERFPP_SPHERICAL) ? r * q.scale : r;
	return (sample_mode == NR3D_NERFPP_BOX || sample_mode == NR3D_NERFPP_CUBE) ? box_t(q, rr) : sphere_t(q, rr);
}

// the radius of shell j of a ray: r, and what the network input is made of (1 / r, log10 r)
struct Radius { float r, r_reci, r_log; };
__device__ __forceinline__ Radius shell_radius(float table, const float *__restrict__ noise_row, uint32_t j, float step, int interval_type) {
	Radius s;
	if (interval_type == NR3D_NERFPP_INVERSE) {
		float v = table;
		if (noise_row) {
			v = table + noise_row[j] * step;
			v = v < 1e-5f ? 1e-5f : v;                     // clamp(1e-5): a NaN stays one
		}
		s.r_reci = v;
		s.r = 1.0f / v;
		s.r_log = 0.0f;
	} else {
		s.r_log = noise_row ? table + noise_row[j] * step : table;
		s.r = powf(10.0f, s.r_log);
		s.r_reci = 1.0f / s.r;
	}
	return s;
}

struct Params {
	uint32_t R, N;
	const float *rays_o, *rays_d, *t_min, *aabb, *radii, *noise;
	float step, last_radius, log_min, log_max;
	int sample_mode, interval_type;
};

// shell j (< N) of the ray: depth, delta, validity
struct Sample { float t, delta; Radius rad; bool valid; };
__device__ __forceinline__ Sample shell_sample(const Params &p, const Ray &q, const float *__restrict__ noise_row, uint32_t j) {
	Sample s;
	s.rad = shell_radius(p.radii[j], noise_row, j, p.step, p.interval_type);
	const float r_next = (j + 1 < p.N) ? shell_radius(p.radii[j + 1], noise_row, j + 1, p.step, p.interval_type).r : p.last_radius;
	s.t = shell_t(q, p.sample_mode, s.rad.r);
	s.delta = shell_t(q, p.sample_mode, r_next) - s.t;
	s.valid = !((s.t != s.t) || (s.t < q.t_min));
	return s;
}

// the 4-D network input of a valid sample
__device__ __forceinline__ float4 network_input(const Params &p, const Ray &q, const Sample &s) {
	float x[3], reci, lg;
	if (p.sample_mode == NR3D_NERFPP_BOX || p.sample_mode == NR3D_NERFPP_ELLIPSOID) {
#pragma unroll
		for (int k = 0; k < 3; ++k) x[k] = fmaf(q.d[k], s.t, q.o[k]) * s.rad.r_reci;
		reci = s.rad.r_reci;
		lg = s.rad.r_log;
	} else {
#pragma unroll
		for (int k = 0; k < 3; ++k) x[k] = (fmaf(q.d[k], s.t, q.o[k]) - q.c[k]) / q.h[k];
		const float n = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
		const float den = n < 1e-12f ? 1e-12f : n;             // F.normalize: x / max(|x|, 1e-12)
#pragma unroll
		for (int k = 0; k < 3; ++k) x[k] = x[k] / den;
		reci = 1.0f / n;
		lg = p.interval_type == NR3D_NERFPP_LOGARITHM ? log10f(n) : 0.0f;
	}
	const float w = p.interval_type == NR3D_NERFPP_LOGARITHM ? (lg - p.log_min) / (p.log_max - p.log_min) * 2.0f - 1.0f
	                                                         : reci * 2.0f - 1.0f;
	return make_float4(x[0], x[1], x[2], w);
}

template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_march(Params p, int64_t *__restrict__ counts, const int64_t *__restrict__ begin_all,
                                                   uint64_t S, float4 *__restrict__ x, float *__restrict__ t,
                                                   float *__restrict__ deltas, int64_t *__restrict__ ridx) {
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t ray = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
	if (ray >= p.R) return;
	const Ray q = load_ray(ray, p.rays_o, p.rays_d, p.t_min, p.aabb, p.sample_mode);
	const float *noise_row = p.noise ? p.noise + (size_t)ray * p.N : nullptr;
	uint64_t base = EMIT ? (uint64_t)begin_all[ray] : 0ull;      // emit: the next free row; count: the shells so far
	for (uint32_t j0 = 0; j0 < p.N; j0 += 64) {
		const uint32_t j = j0 + lane;
		Sample s;
		s.valid = false;
		if (j < p.N) s = shell_sample(p, q, noise_row, j);
		const uint64_t mask = __ballot(s.valid);
		if (EMIT) {
			const uint64_t row = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
			if (s.valid && row < S) {
				x[row] = network_input(p, q, s);
				t[row] = s.t;
				deltas[row] = s.delta;
				ridx[row] = (int64_t)ray;
			}
		}
		base += (uint64_t)__popcll(mask);
	}
	if (!EMIT && lane == 0) counts[ray] = (int64_t)base;
}

static int check_args(const char *fn, uint32_t R, const float *rays_o, const float *rays_d, const float *t_min, const float *aabb, uint32_t N,
                      const float *radii, int sample_mode, int interval_type) {
	NR3D_CHECK(sample_mode >= NR3D_NERFPP_BOX && sample_mode <= NR3D_NERFPP_SPHERICAL,
	           "%s: sample_mode = %d, must be 0 (box), 1 (ellipsoid), 2 (cube) or 3 (spherical)", fn, sample_mode);
	NR3D_CHECK(interval_type >= NR3D_NERFPP_INVERSE && interval_type <= NR3D_NERFPP_LOGARITHM_INV_INPUT,
	           "%s: interval_type = %d, must be 0 (inverse proportional), 1 (logarithm) or 2 (logarithm with inverse input)", fn, interval_type);
	NR3D_CHECK(N >= 1, "%s: a table of N = 0 radii", fn);
	NR3D_CHECK(R < (1u << 28), "%s: R = %u rays, fewer than 2^28 per call", fn, R);
	NR3D_CHECK((uint64_t)R * N < (1ull << 40), "%s: R N = %llu shells, fewer than 2^40 per call", fn, (unsigned long long)R * N);
	NR3D_CHECK(R == 0 || (rays_o && rays_d && t_min), "%s: NULL rays_o / rays_d / t_min", fn);
	NR3D_CHECK(aabb && radii, "%s: NULL aabb / radii", fn);
	return 0;
}

}  // namespace nerfpp
}  // namespace nr3d

using namespace nr3d;

extern "C" int nr3d_nerfpp_march_count(uint32_t R, const float *rays_o, const float *rays_d, const float *t_min, const float *aabb,
                                       uint32_t N, const float *radii, const float *noise, float step, float last_radius, int sample_mode,
                                       int interval_type, float log_min, float log_max, int64_t *counts, void *stream) {
	namespace np = nerfpp;
	NR3D_TRY(np::check_args("nerfpp_march_count", R, rays_o, rays_d, t_min, aabb, N, radii, sample_mode, interval_type));
	if (R == 0) return 0;
	NR3D_CHECK(counts, "nerfpp_march_count: NULL counts");
	const np::Params p{R, N, rays_o, rays_d, t_min, aabb, radii, noise, step, last_radius, log_min, log_max, sample_mode, interval_type};
	hipLaunchKernelGGL(np::k_march<false>, dim3(div_up(R, np::kWaves)), dim3(np::kBlock), 0, (hipStream_t)stream, p, counts,
	                   (const int64_t *)nullptr, (uint64_t)0, (float4 *)nullptr, (float *)nullptr, (float *)nullptr, (int64_t *)nullptr);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_nerfpp_march_emit(uint32_t R, const float *rays_o, const float *rays_d, const float *t_min, const float *aabb,
                                      uint32_t N, const float *radii, const float *noise, float step, float last_radius, int sample_mode,
                                      int interval_type, float log_min, float log_max, const int64_t *begin_all, uint64_t S, float *x,
                                      float *t, float *deltas, int64_t *ridx, void *stream) {
	namespace np = nerfpp;
	NR3D_TRY(np::check_args("nerfpp_march_emit", R, rays_o, rays_d, t_min, aabb, N, radii, sample_mode, interval_type));
	if (R == 0 || S == 0) return 0;
	NR3D_CHECK(begin_all, "nerfpp_march_emit: NULL begin_all");
	NR3D_CHECK(x && t && deltas && ridx, "nerfpp_march_emit: NULL x / t / deltas / ridx");
	NR3D_CHECK(((uintptr_t)x & 15) == 0, "nerfpp_march_emit: x must be 16-byte aligned");
	NR3D_CHECK(S <= (uint64_t)R * N, "nerfpp_march_emit: S = %llu samples from %u rays x %u shells", (unsigned long long)S, R, N);
	const np::Params p{R, N, rays_o, rays_d, t_min, aabb, radii, noise, step, last_radius, log_min, log_max, sample_mode, interval_type};
	hipLaunchKernelGGL(np::k_march<true>, dim3(div_up(R, np::kWaves)), dim3(np::kBlock), 0, (hipStream_t)stream, p, (int64_t *)nullptr,
	                   begin_all, S, (float4 *)x, t, deltas, ridx);
	NR3D_LAUNCH_CHECK();
	return 0;
}
