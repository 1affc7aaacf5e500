// nr3d_lib_amd/csrc/neus_composite.hip -- the last stage of a NeuS render, the volume buffer -> pixels, one launch each way
// (nr3d_neus_composite_fwd / _bwd): vw, mask, depth, rgb and the rendered NORMAL of every ray, on rows ('batched' buffers) and on packs.
//
// The reference runs this as a chain of torch ops at the end of NeusRendererMixin.ray_query (nr3d_lib/models/fields/neus/
// renderer_mixin.py:396-439): ray_alpha_to_vw (roll, cumprod, mul) | packed_alpha_to_vw, then sum / div / mul / index_put per output,
// differentiated by autograd.
//
// PACKS are the device bodies of nr3d_pack_composite_fwd / _bwd (pack_ops.hip) with the normals riding along as a compile-time option;
// without nablas the call IS nr3d_pack_composite_fwd / _bwd.  Early stop, alpha threshold and the reference kernel's backward apply.
//
// ROWS follow ray_alpha_to_vw: w_i = a_i T_i, T_{i+1} = T_i (1 - a_i) over EVERY sample -- no early stop, no threshold (the chain's
// (1 + 1e-10) - a is 1 - a in float32).  A row of n samples is the work of G = min(64, the power of two >= n) neighbouring lanes, 64 / G
// rows per wave, so that the one-sample rows of a sphere-traced buffer fill a wave as the 128-sample rows of an up-sampled one do; rows
// longer than 64 walk in chunks of 64 with T carried.  T is a prefix product (wave_row.h's scan at width G).
// Backward, with g_i = dL/dw_i (comp_gw of pack_ops.hip plus g_normals . nablas_i):
//   dL/da_i = T_i (g_i - R_i),   R_i = g_{i+1} a_{i+1} + (1 - a_{i+1}) R_{i+1},   R_{n-1} = 0
// -- the derivative of the product with the sample's own factor left out, as torch's cumprod backward gives it: no division, so a sample
// with a == 1 gets its exact gradient and so do the ones behind it (T = 0 there).  R is an affine recurrence from the row's end: the maps
// x -> b + m x compose associatively, (m1, b1) o (m2, b2) = (m1 m2, b1 + m1 b2), and are scanned by shuffles like the product.  The chunks
// of a long row are walked from the last to the first with R carried; the T in front of each chunk comes from a forward pass over the
// chunks' products, kept one per lane (64 chunks = 4096 samples; longer rows repeat that pass per 4096 samples).
// Nothing is accumulated across waves, every output element has one writer: the same bits run after run.
#include "common.h"
#include "pack_launch.h"
#include "unit_normal.h"
#include "wave_row.h"

namespace nr3d {
namespace neus_composite {

constexpr int kBlock = 256;

template <int G> __device__ __forceinline__ float group_mul(float v) {
#pragma unroll
	for (int off = G / 2; off >= 1; off >>= 1) v *= __shfl_xor(v, off, G);
	return v;
}
template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
	for (int off = G / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, G);
	return v;
}

// G lanes per row, kBlock / G rows per workgroup.  Every lane of a wave runs every shuffle: a row past the end only loads and stores nothing.
template <int G>
__global__ __launch_bounds__(kBlock) void k_rows_fwd(uint32_t R, uint32_t n, const float *__restrict__ alphas, const float *__restrict__ ts,
                                                     const float *__restrict__ rgb, float *nablas, int normals_mode,
                                                     const int64_t *__restrict__ ray_index, int normalize, float *__restrict__ vw,
                                                     float *__restrict__ mask, float *__restrict__ depth, float *__restrict__ rgb_out,
                                                     float *__restrict__ normals_out) {
	const int gl = threadIdx.x & (G - 1);
	const uint64_t row = (uint64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G;
	const bool valid = row < R;
	const size_t begin = (size_t)row * n;
	float Tc = 1.0f, s = 0.0f, dt = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
	for (uint64_t base = 0; base < n; base += G) {           // 64 bits: n up to 2^32 - 1 must not wrap the counter
		const bool mine = valid && base + gl < n;
		const size_t i = begin + base + gl;
		const float a = mine ? alphas[i] : 0.0f;
		const float t = mine ? ts[i] : 0.0f;
		const float inc = wave_row::incl_mul<G>(1.0f - a, gl);
		float exc = __shfl_up(inc, 1, G);
		if (gl == 0) exc = 1.0f;
		const float w = a * (Tc * exc);
		Tc *= __shfl(inc, G - 1, G);
		if (mine) vw[i] = w;
		s += w; dt += w * t;
		if (rgb && mine) { c0 += w * rgb[3 * i]; c1 += w * rgb[3 * i + 1]; c2 += w * rgb[3 * i + 2]; }
		if (nablas && mine) {
			const V3 v = load_normal(nablas, i, normals_mode);
			m0 += w * v.x; m1 += w * v.y; m2 += w * v.z;
		}
	}
	s = group_sum<G>(s); dt = group_sum<G>(dt);
	if (rgb) { c0 = group_sum<G>(c0); c1 = group_sum<G>(c1); c2 = group_sum<G>(c2); }
	if (nablas) { m0 = group_sum<G>(m0); m1 = group_sum<G>(m1); m2 = group_sum<G>(m2); }
	if (valid && gl == 0) {
		const size_t o = ray_index ? (size_t)ray_index[row] : (size_t)row;
		mask[o] = s;
		depth[o] = normalize ? dt / (s + 1e-10f) : dt;
		if (rgb) { rgb_out[3 * o] = c0; rgb_out[3 * o + 1] = c1; rgb_out[3 * o + 2] = c2; }
		if (nablas) { normals_out[3 * o] = m0; normals_out[3 * o + 1] = m1; normals_out[3 * o + 2] = m2; }
	}
}

// nablas is read only where g_normals is given; normals_mode 1 never comes here with g_normals or grad_nablas (the entry refuses it)
template <int G>
__global__ __launch_bounds__(kBlock) void k_rows_bwd(uint32_t R, uint32_t n, const float *__restrict__ alphas, const float *__restrict__ vw,
                                                     const float *__restrict__ ts, const float *__restrict__ rgb,
                                                     const float *__restrict__ nablas, const int64_t *__restrict__ ray_index, int normalize,
                                                     const float *__restrict__ mask, const float *__restrict__ depth,
                                                     const float *__restrict__ g_mask, const float *__restrict__ g_depth,
                                                     const float *__restrict__ g_rgb, const float *__restrict__ g_normals,
                                                     const float *__restrict__ g_vw, float *__restrict__ grad_alphas,
                                                     float *__restrict__ grad_t, float *__restrict__ grad_rgb,
                                                     float *__restrict__ grad_nablas) {
	const int gl = threadIdx.x & (G - 1);
	const uint64_t row = (uint64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G;
	const bool valid = row < R;
	const size_t begin = (size_t)row * n;
	// the per-ray grads: dL/dw_i = gm + cd (t_i - dref) + g_rgb . rgb_i + g_normals . nablas_i + g_vw_i
	float gm = 0.0f, cd = 0.0f, dref = 0.0f, q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
	if (valid) {
		const size_t o = ray_index ? (size_t)ray_index[row] : (size_t)row;
		const float gd = g_depth ? g_depth[o] : 0.0f;
		gm = g_mask ? g_mask[o] : 0.0f;
		cd = normalize ? gd / (mask[o] + 1e-10f) : gd;
		dref = normalize ? depth[o] : 0.0f;
		if (g_rgb && rgb) { q0 = g_rgb[3 * o]; q1 = g_rgb[3 * o + 1]; q2 = g_rgb[3 * o + 2]; }
		if (g_normals) { n0 = g_normals[3 * o]; n1 = g_normals[3 * o + 1]; n2 = g_normals[3 * o + 2]; }
	}
	const uint64_t chunks = ((uint64_t)n + G - 1) / G;
	float Rc = 0.0f;                                         // R in front of the chunks already walked (behind them in the row)
	for (uint64_t sb = (chunks + G - 1) / G; sb-- > 0;) {    // G chunks at a time, from the row's end
		const uint64_t c_first = sb * G, c_end = (sb + 1) * G < chunks ? (sb + 1) * G : chunks;
		// T in front of chunk c_first + gl, into lane gl.  The walk starts at the row's first chunk for every group of G chunks: a row
		// of n <= 64 G = 4096 samples pays it once, a longer one n / 4096 times over (quadratic in n / 4096; volume buffers have rows of
		// tens to hundreds of samples, and the T of a group's start cannot be carried while the groups are taken from the row's end)
		float Tc = 1.0f, Tstart = 1.0f;
		for (uint64_t c = 0; c < c_end; ++c) {
			if (c == c_first + gl) Tstart = Tc;
			if (c + 1 < c_end) {
				const uint64_t j = c * G + gl;
				Tc *= group_mul<G>((valid && j < n) ? 1.0f - alphas[begin + j] : 1.0f);
			}
		}
		for (uint64_t c = c_end; c-- > c_first;) {
			const uint64_t j = c * G + gl;
			const bool mine = valid && j < n;
			const size_t i = begin + j;
			const float a = mine ? alphas[i] : 0.0f;
			const float w = mine ? vw[i] : 0.0f;
			float g = 0.0f;
			if (mine) {
				g = __fmaf_rn(cd, ts[i] - dref, gm);
				if (g_rgb && rgb) { g = __fmaf_rn(q0, rgb[3 * i], g); g = __fmaf_rn(q1, rgb[3 * i + 1], g); g = __fmaf_rn(q2, rgb[3 * i + 2], g); }
				if (g_normals) { g = __fmaf_rn(n0, nablas[3 * i], g); g = __fmaf_rn(n1, nablas[3 * i + 1], g); g = __fmaf_rn(n2, nablas[3 * i + 2], g); }
				if (g_vw) g += g_vw[i];
			}
			const float inc = wave_row::incl_mul<G>(1.0f - a, gl);
			float exc = __shfl_up(inc, 1, G);
			if (gl == 0) exc = 1.0f;
			const float Tin = __shfl(Tstart, (int)(c - c_first), G) * exc;
			// the maps x -> B + M x of the samples from mine to the chunk's last, composed
			float M = 1.0f - a, B = g * a;
#pragma unroll
			for (int off = 1; off < G; off <<= 1) {
				const float Mo = __shfl_down(M, off, G), Bo = __shfl_down(B, off, G);
				if (gl + off < G) { B = __fmaf_rn(M, Bo, B); M *= Mo; }
			}
			const float V = __fmaf_rn(M, Rc, B);
			float Rn = __shfl_down(V, 1, G);                 // R_i = the composed map of sample i + 1 at Rc
			if (gl == G - 1) Rn = Rc;
			Rc = __shfl(V, 0, G);
			if (mine) {
				grad_alphas[i] = Tin * (g - Rn);
				if (grad_t) grad_t[i] = cd * w;
				if (grad_rgb) { grad_rgb[3 * i] = w * q0; grad_rgb[3 * i + 1] = w * q1; grad_rgb[3 * i + 2] = w * q2; }
				if (grad_nablas) { grad_nablas[3 * i] = w * n0; grad_nablas[3 * i + 1] = w * n1; grad_nablas[3 * i + 2] = w * n2; }
			}
		}
	}
}

// lanes per row: the power of two >= n, at most a wave.  -DNR3D_NEUS_ROWS_MIN_LANES=64 builds the alternative that was measured against
// it, a whole wave per row whatever n (profiles/neus_composite.json, lane_mapping)
#ifndef NR3D_NEUS_ROWS_MIN_LANES
#define NR3D_NEUS_ROWS_MIN_LANES 1
#endif
static inline int lanes_for(uint32_t n) {
	int g = NR3D_NEUS_ROWS_MIN_LANES;
	while (g < 64 && (uint32_t)g < n) g <<= 1;
	return g;
}

// what both directions check before any launch
static int check_args(const char *fn, int layout, uint32_t P, uint64_t S, uint32_t n, const float *alphas, const float *t,
                      const int64_t *pack_infos, int normals_mode) {
	NR3D_CHECK(layout == NR3D_NEUS_COMPOSITE_ROWS || layout == NR3D_NEUS_COMPOSITE_PACKED, "%s: layout = %d, must be 0 (rows) or 1 (packs)", fn,
	           layout);
	NR3D_CHECK(normals_mode == 0 || normals_mode == 1, "%s: normals_mode = %d, must be 0 (raw) or 1 (clamped and normalised)", fn, normals_mode);
	NR3D_CHECK(S < (1ull << 32), "%s: S = %llu, at most 2^32 - 1 samples per call", fn, (unsigned long long)S);
	if (layout == NR3D_NEUS_COMPOSITE_ROWS) {
		NR3D_CHECK(!pack_infos, "%s: rows take no pack_infos", fn);
		NR3D_CHECK(P == 0 || n >= 1, "%s: rows of n = 0 samples", fn);
		NR3D_CHECK((uint64_t)P * n == S, "%s: rows layout with P * n = %u * %u != S = %llu", fn, P, n, (unsigned long long)S);
	} else {
		NR3D_CHECK(P == 0 || pack_infos, "%s: NULL pack_infos", fn);
	}
	NR3D_CHECK(P == 0 || S == 0 || (alphas && t), "%s: NULL alphas or t", fn);
	return 0;
}

#define NR3D_ROWS_DISPATCH(G, LAUNCH) switch (G) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 4: LAUNCH(4); break; \
	case 8: LAUNCH(8); break; case 16: LAUNCH(16); break; case 32: LAUNCH(32); break; default: LAUNCH(64); break; }

}  // namespace neus_composite
}  // namespace nr3d

using namespace nr3d;

extern "C" int nr3d_neus_composite_fwd(int layout, uint32_t P, uint64_t S, uint32_t n, const float *alphas, const float *t, const float *rgb,
                                       float *nablas, const int64_t *pack_infos, const int64_t *ray_index, float early_stop_eps,
                                       float alpha_thre, int normalize_depth, int normals_mode, float *vw, float *mask, float *depth,
                                       float *rgb_out, float *normals_out, void *stream) {
	namespace nc = neus_composite;
	NR3D_TRY(nc::check_args("neus_composite_fwd", layout, P, S, n, alphas, t, pack_infos, normals_mode));
	if (P == 0) return 0;
	NR3D_CHECK(mask && depth && (S == 0 || vw), "neus_composite_fwd: NULL vw, mask or depth");
	NR3D_CHECK(!rgb || rgb_out, "neus_composite_fwd: rgb given without rgb_out");
	NR3D_CHECK(!nablas || normals_out, "neus_composite_fwd: nablas given without normals_out");
	hipStream_t st = (hipStream_t)stream;
	if (layout == NR3D_NEUS_COMPOSITE_PACKED) {
		if (!nablas)
			return nr3d_pack_composite_fwd(P, alphas, t, rgb, pack_infos, ray_index, early_stop_eps, alpha_thre, normalize_depth, vw, mask,
			                               depth, rgb_out, stream);
		return pk::launch_neus_composite_packs_fwd(P, alphas, t, rgb, nablas, normals_mode, pack_infos, ray_index, early_stop_eps, alpha_thre,
		                                           normalize_depth, vw, mask, depth, rgb_out, normals_out, st);
	}
	const int G = nc::lanes_for(n);
	const dim3 grid(div_up(P, nc::kBlock / G)), block(nc::kBlock);
#define NR3D_ROWS_FWD(GG) hipLaunchKernelGGL(nc::k_rows_fwd<GG>, grid, block, 0, st, P, n, alphas, t, rgb, nablas, normals_mode, ray_index, \
	normalize_depth, vw, mask, depth, rgb_out, normals_out)
	NR3D_ROWS_DISPATCH(G, NR3D_ROWS_FWD)
#undef NR3D_ROWS_FWD
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_neus_composite_bwd(int layout, uint32_t P, uint64_t S, uint32_t n, const float *alphas, const float *t, const float *rgb,
                                       const float *nablas, const int64_t *pack_infos, const int64_t *ray_index, float early_stop_eps,
                                       float alpha_thre, int normalize_depth, int normals_mode, const float *vw, const float *mask,
                                       const float *depth, const float *g_mask, const float *g_depth, const float *g_rgb,
                                       const float *g_normals, const float *g_vw, float *grad_alphas, float *grad_t, float *grad_rgb,
                                       float *grad_nablas, void *stream) {
	namespace nc = neus_composite;
	NR3D_TRY(nc::check_args("neus_composite_bwd", layout, P, S, n, alphas, t, pack_infos, normals_mode));
	NR3D_CHECK(normals_mode == 0 || (!g_normals && !grad_nablas),
	           "neus_composite_bwd: normals_mode 1 (clamped and normalised normals) is forward only: no g_normals, no grad_nablas");
	NR3D_CHECK((!g_normals && !grad_nablas) || nablas, "neus_composite_bwd: g_normals or grad_nablas without nablas");
	NR3D_CHECK(!grad_rgb || rgb, "neus_composite_bwd: grad_rgb without rgb");
	if (P == 0) return 0;
	NR3D_CHECK(mask && depth && (S == 0 || (vw && grad_alphas)), "neus_composite_bwd: NULL vw, mask, depth or grad_alphas");
	hipStream_t st = (hipStream_t)stream;
	if (layout == NR3D_NEUS_COMPOSITE_PACKED) {
		if (!g_normals && !grad_nablas)
			return nr3d_pack_composite_bwd(P, alphas, vw, t, rgb, pack_infos, ray_index, early_stop_eps, alpha_thre, normalize_depth, mask, depth,
			                               g_mask, g_depth, g_rgb, g_vw, grad_alphas, grad_t, grad_rgb, stream);
		return pk::launch_neus_composite_packs_bwd(P, alphas, vw, t, rgb, nablas, pack_infos, ray_index, early_stop_eps, alpha_thre,
		                                           normalize_depth, mask, depth, g_mask, g_depth, g_rgb, g_normals, g_vw, grad_alphas, grad_t,
		                                           grad_rgb, grad_nablas, st);
	}
	const int G = nc::lanes_for(n);
	const dim3 grid(div_up(P, nc::kBlock / G)), block(nc::kBlock);
#define NR3D_ROWS_BWD(GG) hipLaunchKernelGGL(nc::k_rows_bwd<GG>, grid, block, 0, st, P, n, alphas, vw, t, rgb, nablas, ray_index, \
	normalize_depth, mask, depth, g_mask, g_depth, g_rgb, g_normals, g_vw, grad_alphas, grad_t, grad_rgb, grad_nablas)
	NR3D_ROWS_DISPATCH(G, NR3D_ROWS_BWD)
#undef NR3D_ROWS_BWD
	NR3D_LAUNCH_CHECK();
	return 0;
}
