// nr3d_lib_amd/csrc/embed.hip -- the two small embedders of the reference (externals/shencoder, externals/freqencoder) for gfx950:
// real spherical harmonics of a direction and the sinusoidal embedding, forward, backward and (frequency only) double backward.
// Entry points: nr3d_sh_encode_* / nr3d_freq_encode_* of include/nr3d_hip.h.
//
// Both are element-wise and memory bound, so the kernels are organised around their stores:
//   * SH: one wave per 64 points.  A lane evaluates its point (arithmetic in fp32 for both dtypes) into an LDS tile with an odd row
//     pitch (no bank conflicts), then the wave writes the tile to memory row by row with consecutive lanes on consecutive addresses,
//     16 bytes per lane where the row length, the row stride and the pointer allow.  The backward reads dL/dy the same way and
//     RECOMPUTES the derivatives from x (12 + 4 C^2 + 12 bytes per point) unless the caller hands in a stored Jacobian.
//   * frequency: one lane per four consecutive outputs of the flat [B, C] array (one 16-byte store), or one lane per output when the
//     rows are a slice of a wider buffer.
// No atomics, no workspace, no host wait; everything runs on the caller's stream.  Same bytes run after run.
#include "common.h"
#include "sh_basis.inc"

namespace nr3d {
namespace embed {

constexpr int kTile = 64;       // points per workgroup = one wave

// ---- spherical harmonics -------------------------------------------------------------------------------------------------------
// f(c, Y_c, dY_c/dx, dY_c/dy, dY_c/dz) for every column c = l^2 + l + m, l < DEG.  (x + iy)^a by its recurrence (two roundings per
// step), s K Q_l^a(z) and its z-derivative by Horner's rule in z^2 on the generated coefficients.  Everything is unrolled: the
// coefficients are immediates and what a caller's functor ignores is never computed.  Roundings on the longest path of one monomial:
// 14 for a value (a = 7: 12 in the recurrence, one in the coefficient, one in the product), 15 for a derivative.
template <int DEG, typename F>
__device__ __forceinline__ void sh_eval(float x, float y, float z, F &&f) {
	const float z2 = z * z;
	float cr = 1.f, ci = 0.f;       // (x + iy)^a
	float pr = 0.f, pi = 0.f;       // (x + iy)^(a-1)
#pragma unroll
	for (int a = 0; a < DEG; ++a) {
		if (a == 1) { pr = 1.f; pi = 0.f; cr = x; ci = y; }
		if (a > 1) {
			pr = cr; pi = ci;
			cr = fmaf(x, pr, -(y * pi));
			ci = fmaf(x, pi, y * pr);
		}
#pragma unroll
		for (int l = a; l < DEG; ++l) {
			const int nv = (l - a) / 2 + 1;
			float q = SH_V[l][a][0];
#pragma unroll
			for (int t = 1; t < nv; ++t) q = fmaf(q, z2, SH_V[l][a][t]);
			if ((l - a) & 1) q *= z;
			float qz = 0.f;
			if (a < l) {
				const int nz = (l - a - 1) / 2 + 1;
				qz = SH_Z[l][a][0];
#pragma unroll
				for (int t = 1; t < nz; ++t) qz = fmaf(qz, z2, SH_Z[l][a][t]);
				if ((l - a - 1) & 1) qz *= z;
			}
			if (a == 0) {
				f(l * l + l, q, 0.f, 0.f, qz);
			} else {
				const float aq = (float)a * q;
				f(l * l + l + a, q * cr, aq * pr, -(aq * pi), qz * cr);
				f(l * l + l - a, q * ci, aq * pi, aq * pr, qz * ci);
			}
		}
	}
}

template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int N = 4; };
template <> struct Vec16<__half> { static constexpr int N = 8; };

// the LDS tile [rows][W] (row pitch P floats) -> out[(row0 + r) * stride + c], consecutive lanes on consecutive addresses
template <typename T, int W, int P>
__device__ __forceinline__ void tile_store(const float *tile, T *out, int64_t stride, uint64_t row0, uint32_t rows, bool vec, int lane) {
	constexpr int N = Vec16<T>::N;
	if (W % N == 0 && vec) {
		constexpr int WV = (W % N == 0) ? W / N : 1;
		for (uint32_t i = lane; i < rows * WV; i += kTile) {
			const uint32_t r = i / WV, c = (i % WV) * N;
			const float *s = tile + r * P + c;
			alignas(16) T v[N];
#pragma unroll
			for (int k = 0; k < N; ++k) v[k] = from_f32<T>(s[k]);
			*reinterpret_cast<uint4 *>(out + (row0 + r) * stride + c) = *reinterpret_cast<const uint4 *>(v);
		}
	} else {
		for (uint32_t i = lane; i < rows * W; i += kTile) {
			const uint32_t r = i / W, c = i % W;
			out[(row0 + r) * stride + c] = from_f32<T>(tile[r * P + c]);
		}
	}
}

template <typename T, int W, int P>
__device__ __forceinline__ void tile_load(float *tile, const T *in, int64_t stride, uint64_t row0, uint32_t rows, bool vec, int lane) {
	constexpr int N = Vec16<T>::N;
	if (W % N == 0 && vec) {
		constexpr int WV = (W % N == 0) ? W / N : 1;
		for (uint32_t i = lane; i < rows * WV; i += kTile) {
			const uint32_t r = i / WV, c = (i % WV) * N;
			alignas(16) T v[N];
			*reinterpret_cast<uint4 *>(v) = *reinterpret_cast<const uint4 *>(in + (row0 + r) * stride + c);
			float *d = tile + r * P + c;
#pragma unroll
			for (int k = 0; k < N; ++k) d[k] = to_f32<T>(v[k]);
		}
	} else {
		for (uint32_t i = lane; i < rows * W; i += kTile) {
			const uint32_t r = i / W, c = i % W;
			tile[r * P + c] = to_f32<T>(in[(row0 + r) * stride + c]);
		}
	}
}

template <typename T, int DEG>
__global__ void __launch_bounds__(kTile) k_sh_fwd(uint64_t B, const T *__restrict__ xin, T *__restrict__ yout, int64_t y_stride, bool y_vec,
                                                  T *__restrict__ jac, bool jac_vec) {
	constexpr int W = DEG * DEG, P = W | 1;
	__shared__ float tile[kTile * P];
	const int lane = threadIdx.x;
	const uint64_t row0 = (uint64_t)blockIdx.x * kTile;
	const uint32_t rows = (uint32_t)min((uint64_t)kTile, B - row0);
	float x = 0.f, y = 0.f, z = 0.f;
	if (lane < (int)rows) {
		const T *p = xin + (row0 + lane) * 3;
		x = to_f32<T>(p[0]); y = to_f32<T>(p[1]); z = to_f32<T>(p[2]);
	}
	float *mine = tile + lane * P;
	sh_eval<DEG>(x, y, z, [&](int c, float v, float, float, float) { mine[c] = v; });
	__syncthreads();
	tile_store<T, W, P>(tile, yout, y_stride, row0, rows, y_vec, lane);
	if (jac == nullptr) return;
	// the stored-Jacobian route (the reference's layout [B, 3, C^2]): one pass of the tile per input dimension
	for (int d = 0; d < 3; ++d) {
		__syncthreads();
		if (d == 0) sh_eval<DEG>(x, y, z, [&](int c, float, float dx, float, float) { mine[c] = dx; });
		else if (d == 1) sh_eval<DEG>(x, y, z, [&](int c, float, float, float dy, float) { mine[c] = dy; });
		else sh_eval<DEG>(x, y, z, [&](int c, float, float, float, float dz) { mine[c] = dz; });
		__syncthreads();
		tile_store<T, W, P>(tile, jac + d * W, 3 * W, row0, rows, jac_vec, lane);
	}
}

// dL/dx[b, d] (+)= sum_c g[b, c] dY_c/dx_d; the derivatives recomputed from x (jac == nullptr) or read from the stored Jacobian
template <typename T, int DEG>
__global__ void __launch_bounds__(kTile) k_sh_bwd(uint64_t B, const T *__restrict__ grad, int64_t g_stride, bool g_vec, const T *__restrict__ xin,
                                                  const T *__restrict__ jac, bool jac_vec, T *__restrict__ gx, bool accumulate) {
	constexpr int W = DEG * DEG, P = W | 1;
	__shared__ float gt[kTile * P];
	__shared__ float jt[kTile * P];
	const int lane = threadIdx.x;
	const uint64_t row0 = (uint64_t)blockIdx.x * kTile;
	const uint32_t rows = (uint32_t)min((uint64_t)kTile, B - row0);
	tile_load<T, W, P>(gt, grad, g_stride, row0, rows, g_vec, lane);
	__syncthreads();
	const bool live = lane < (int)rows;
	const float *g = gt + lane * P;
	float s[3] = {0.f, 0.f, 0.f};
	if (jac == nullptr) {
		if (live) {
			const T *p = xin + (row0 + lane) * 3;
			sh_eval<DEG>(to_f32<T>(p[0]), to_f32<T>(p[1]), to_f32<T>(p[2]), [&](int c, float, float dx, float dy, float dz) {
				s[0] = fmaf(g[c], dx, s[0]); s[1] = fmaf(g[c], dy, s[1]); s[2] = fmaf(g[c], dz, s[2]);
			});
		}
	} else {
		for (int d = 0; d < 3; ++d) {
			tile_load<T, W, P>(jt, jac + d * W, 3 * W, row0, rows, jac_vec, lane);
			__syncthreads();
			if (live) {
				const float *j = jt + lane * P;
				float a = 0.f;
#pragma unroll
				for (int c = 0; c < W; ++c) a = fmaf(g[c], j[c], a);
				s[d] = a;
			}
			__syncthreads();
		}
	}
	if (live) {
		T *o = gx + (row0 + lane) * 3;
#pragma unroll
		for (int d = 0; d < 3; ++d) o[d] = from_f32<T>(accumulate ? to_f32<T>(o[d]) + s[d] : s[d]);
	}
}

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

template <typename T, int DEG>
static int sh_fwd_launch(uint64_t B, const void *x, void *y, int64_t y_stride, void *jac, hipStream_t st) {
	constexpr int N = Vec16<T>::N;
	const bool y_vec = aligned16(y) && y_stride % N == 0;
	hipLaunchKernelGGL((k_sh_fwd<T, DEG>), dim3(div_up(B, kTile)), dim3(kTile), 0, st, B, (const T *)x, (T *)y, y_stride, y_vec, (T *)jac,
	                   aligned16(jac));
	NR3D_LAUNCH_CHECK();
	return 0;
}

template <typename T, int DEG>
static int sh_bwd_launch(uint64_t B, const void *g, int64_t g_stride, const void *x, const void *jac, void *gx, bool acc, hipStream_t st) {
	constexpr int N = Vec16<T>::N;
	const bool g_vec = aligned16(g) && g_stride % N == 0;
	hipLaunchKernelGGL((k_sh_bwd<T, DEG>), dim3(div_up(B, kTile)), dim3(kTile), 0, st, B, (const T *)g, g_stride, g_vec, (const T *)x,
	                   (const T *)jac, aligned16(jac), (T *)gx, acc);
	NR3D_LAUNCH_CHECK();
	return 0;
}

#define NR3D_SH_DISPATCH(T, fn, ...)                                                                                                   \
	switch (degree) {                                                                                                                  \
	case 1: return fn<T, 1>(__VA_ARGS__); case 2: return fn<T, 2>(__VA_ARGS__); case 3: return fn<T, 3>(__VA_ARGS__);                  \
	case 4: return fn<T, 4>(__VA_ARGS__); case 5: return fn<T, 5>(__VA_ARGS__); case 6: return fn<T, 6>(__VA_ARGS__);                  \
	case 7: return fn<T, 7>(__VA_ARGS__); default: return fn<T, 8>(__VA_ARGS__);                                                       \
	}

// ---- frequency embedding -------------------------------------------------------------------------------------------------------
// column c of row b: x[c] for c < D, else sin(2^f x_d + k pi/2) with col = c / D - 1, d = c % D, f = col / 2, k = col % 2: the argument
// is formed in fp32 exactly as the reference does (the scaling is exact, the phase is one rounded add), the sine is the accurate one
// (the only route built and measured; DESIGN 4e says what else was considered).  DD: D when it is 1..4 (divisions by a constant), 0: the runtime value.
template <int DD>
__device__ __forceinline__ float freq_elem(const float *__restrict__ x, uint32_t b, uint32_t c, uint32_t Drt) {
	const uint32_t D = DD ? (uint32_t)DD : Drt;
	const float *row = x + (uint64_t)b * D;
	if (c < D) return row[c];
	const uint32_t col = c / D - 1, d = c % D;
	const float arg = ldexpf(row[d], (int)(col >> 1)) + ((col & 1u) ? 1.57079632679489662f : 0.f);
	return sinf(arg);
}

// contiguous rows: lane t writes the flat elements 4t .. 4t + 3 with one 16-byte store
template <int DD>
__global__ void __launch_bounds__(256) k_freq_fwd_flat(uint32_t total, uint32_t D, uint32_t C, const float *__restrict__ x, float *__restrict__ y) {
	const uint32_t e = (blockIdx.x * 256u + threadIdx.x) * 4u;
	if (e >= total) return;
	uint32_t b = e / C, c = e - b * C;
	float v[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		v[i] = (e + i < total) ? freq_elem<DD>(x, b, c, D) : 0.f;
		if (++c == C) { c = 0; ++b; }
	}
	if (e + 4 <= total) {
		*reinterpret_cast<float4 *>(y + e) = make_float4(v[0], v[1], v[2], v[3]);
	} else {
		for (uint32_t i = 0; e + i < total; ++i) y[e + i] = v[i];
	}
}

// rows that are a column slice of a wider buffer (or an unaligned base): one lane per element, consecutive lanes along a row
template <int DD>
__global__ void __launch_bounds__(256) k_freq_fwd_rows(uint32_t total, uint32_t D, uint32_t C, const float *__restrict__ x, float *__restrict__ y,
                                                       int64_t y_stride) {
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	if (e >= total) return;
	const uint32_t b = e / C, c = e - b * C;
	y[(uint64_t)b * y_stride + c] = freq_elem<DD>(x, b, c, D);
}

// dL/dx from the saved outputs, no trigonometry: d/dx sin(2^f x) = 2^f cos(2^f x) = 2^f y_{f,1}, d/dx cos(2^f x) = -2^f y_{f,0}
__global__ void __launch_bounds__(256) k_freq_bwd(uint32_t total, uint32_t D, uint32_t n_freq, uint32_t C, const float *__restrict__ grad,
                                                  const float *__restrict__ y, int64_t y_stride, float *__restrict__ gx) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t >= total) return;
	const uint32_t b = t / D, d = t - b * D;
	const float *g = grad + (uint64_t)b * C + d, *o = y + (uint64_t)b * y_stride + d;
	float acc = g[0];
	for (uint32_t f = 0; f < n_freq; ++f) {
		const uint32_t c0 = D + 2u * f * D, c1 = c0 + D;
		acc = fmaf(ldexpf(1.f, (int)f), fmaf(g[c0], o[c1], -(g[c1] * o[c0])), acc);
	}
	gx[t] = acc;
}

// the backward of the backward: with v = dL/d(gx),  dL/dg_d = v_d,  dL/dg_{f,0,d} = v_d 2^f y_{f,1,d},  dL/dg_{f,1,d} = -v_d 2^f y_{f,0,d},
// dL/dx_d = -v_d sum_f 4^f (g_{f,0,d} y_{f,0,d} + g_{f,1,d} y_{f,1,d}).  DG: one lane per element of dL/dg [B, C] (the lanes of the
// identity columns also sum dL/dx when DX); !DG: one lane per element of dL/dx [B, D].
template <bool DG, bool DX>
__global__ void __launch_bounds__(256) k_freq_bwd_bwd(uint32_t total, uint32_t D, uint32_t n_freq, uint32_t C, const float *__restrict__ v,
                                                      const float *__restrict__ grad, const float *__restrict__ y, int64_t y_stride,
                                                      float *__restrict__ d_grad, float *__restrict__ d_x) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t >= total) return;
	const uint32_t W = DG ? C : D;
	const uint32_t b = t / W, c = t - b * W;
	const float *o = y + (uint64_t)b * y_stride;
	if (c < D) {
		const float vd = v[(uint64_t)b * D + c];
		if (DG) d_grad[t] = vd;
		if (DX) {
			const float *g = grad + (uint64_t)b * C;
			float s = 0.f;
			for (uint32_t f = 0; f < n_freq; ++f) {
				const uint32_t c0 = D + 2u * f * D + c, c1 = c0 + D;
				s = fmaf(ldexpf(1.f, 2 * (int)f), fmaf(g[c0], o[c0], g[c1] * o[c1]), s);
			}
			d_x[(uint64_t)b * D + c] = -(vd * s);
		}
	} else if (DG) {
		const uint32_t col = c / D - 1, d = c - (col + 1) * D;
		const float vs = v[(uint64_t)b * D + d] * ldexpf(1.f, (int)(col >> 1));
		d_grad[t] = (col & 1u) ? -(vs * o[c - D]) : vs * o[c + D];
	}
}

template <int DD>
static int freq_fwd_launch(uint32_t total, uint32_t D, uint32_t C, const float *x, float *y, int64_t y_stride, hipStream_t st) {
	if (y_stride == (int64_t)C && aligned16(y))
		hipLaunchKernelGGL(k_freq_fwd_flat<DD>, dim3(div_up(div_up(total, 4), 256)), dim3(256), 0, st, total, D, C, x, y);
	else
		hipLaunchKernelGGL(k_freq_fwd_rows<DD>, dim3(div_up(total, 256)), dim3(256), 0, st, total, D, C, x, y, y_stride);
	NR3D_LAUNCH_CHECK();
	return 0;
}

static int freq_check(const char *fn, uint64_t B, uint32_t D, uint32_t n_freq, uint32_t C) {
	NR3D_CHECK(D >= 1, "%s: D must be at least 1", fn);
	// 2^f x + k pi/2 in fp32: from f = 24 on one unit in the last place of the argument of an |x| ~ 1 is 2 or more, larger than the phase
	// pi/2 itself, so the two columns of such a frequency no longer differ; 4^f of the double backward is far from overflow there
	NR3D_CHECK(n_freq <= 24, "%s: n_freq = %u, at most 24 frequencies (2^f x + pi/2 has no phase left in fp32 beyond)", fn, n_freq);
	NR3D_CHECK((uint64_t)C == (uint64_t)D + 2ull * D * n_freq, "%s: C = %u, expected D + 2 D n_freq = %llu", fn, C,
	           (unsigned long long)((uint64_t)D + 2ull * D * n_freq));
	NR3D_CHECK(B < (1ull << 31) && B * (uint64_t)C < (1ull << 31), "%s: B * C = %llu, at most 2^31 - 1 elements per call (split the batch)", fn,
	           (unsigned long long)(B * (uint64_t)C));
	return 0;
}

}  // namespace embed
}  // namespace nr3d

using namespace nr3d;

extern "C" int nr3d_sh_encode_fwd(uint64_t B, uint32_t D, uint32_t degree, int dtype, const void *x, void *y, int64_t y_stride, void *dy_dx,
                                  void *stream) {
	NR3D_CHECK(D == 3, "sh_encode_fwd: D = %u, the SH embedder takes 3-D inputs", D);
	NR3D_CHECK(degree >= 1 && degree <= NR3D_SH_MAX_DEGREE, "sh_encode_fwd: degree = %u, must be in [1, 8]", degree);
	NR3D_CHECK(dtype == NR3D_F32 || dtype == NR3D_F16, "sh_encode_fwd: dtype %d, float32 or float16 only", dtype);
	NR3D_CHECK(y_stride >= (int64_t)(degree * degree), "sh_encode_fwd: y_stride = %lld is smaller than a row of %u", (long long)y_stride,
	           degree * degree);
	NR3D_CHECK(B < (1ull << 31), "sh_encode_fwd: B = %llu, at most 2^31 - 1 rows per call", (unsigned long long)B);
	if (B == 0) return 0;
	NR3D_CHECK(x && y, "sh_encode_fwd: NULL tensor pointer");
	hipStream_t st = (hipStream_t)stream;
	if (dtype == NR3D_F32) { NR3D_SH_DISPATCH(float, embed::sh_fwd_launch, B, x, y, y_stride, dy_dx, st) }
	NR3D_SH_DISPATCH(__half, embed::sh_fwd_launch, B, x, y, y_stride, dy_dx, st)
}

extern "C" int nr3d_sh_encode_bwd(uint64_t B, uint32_t D, uint32_t degree, int dtype, const void *grad, int64_t grad_stride, const void *x,
                                  const void *dy_dx, void *grad_x, int accumulate, void *stream) {
	NR3D_CHECK(D == 3, "sh_encode_bwd: D = %u, the SH embedder takes 3-D inputs", D);
	NR3D_CHECK(degree >= 1 && degree <= NR3D_SH_MAX_DEGREE, "sh_encode_bwd: degree = %u, must be in [1, 8]", degree);
	NR3D_CHECK(dtype == NR3D_F32 || dtype == NR3D_F16, "sh_encode_bwd: dtype %d, float32 or float16 only", dtype);
	NR3D_CHECK(grad_stride >= (int64_t)(degree * degree), "sh_encode_bwd: grad_stride = %lld is smaller than a row of %u",
	           (long long)grad_stride, degree * degree);
	NR3D_CHECK(B < (1ull << 31), "sh_encode_bwd: B = %llu, at most 2^31 - 1 rows per call", (unsigned long long)B);
	if (B == 0) return 0;
	NR3D_CHECK(grad && grad_x && (x || dy_dx), "sh_encode_bwd: NULL tensor pointer (x may be NULL only with a stored dy_dx)");
	hipStream_t st = (hipStream_t)stream;
	const bool acc = accumulate != 0;
	if (dtype == NR3D_F32) { NR3D_SH_DISPATCH(float, embed::sh_bwd_launch, B, grad, grad_stride, x, dy_dx, grad_x, acc, st) }
	NR3D_SH_DISPATCH(__half, embed::sh_bwd_launch, B, grad, grad_stride, x, dy_dx, grad_x, acc, st)
}

extern "C" int nr3d_freq_encode_fwd(uint64_t B, uint32_t D, uint32_t n_freq, uint32_t C, const float *x, float *y, int64_t y_stride,
                                    void *stream) {
	if (embed::freq_check("freq_encode_fwd", B, D, n_freq, C)) return 1;
	NR3D_CHECK(y_stride >= (int64_t)C, "freq_encode_fwd: y_stride = %lld is smaller than a row of %u", (long long)y_stride, C);
	if (B == 0) return 0;
	NR3D_CHECK(x && y, "freq_encode_fwd: NULL tensor pointer");
	hipStream_t st = (hipStream_t)stream;
	const uint32_t total = (uint32_t)(B * C);
	switch (D) {
	case 1: return embed::freq_fwd_launch<1>(total, D, C, x, y, y_stride, st);
	case 2: return embed::freq_fwd_launch<2>(total, D, C, x, y, y_stride, st);
	case 3: return embed::freq_fwd_launch<3>(total, D, C, x, y, y_stride, st);
	case 4: return embed::freq_fwd_launch<4>(total, D, C, x, y, y_stride, st);
	default: return embed::freq_fwd_launch<0>(total, D, C, x, y, y_stride, st);
	}
}

extern "C" int nr3d_freq_encode_bwd(uint64_t B, uint32_t D, uint32_t n_freq, uint32_t C, const float *grad, const float *y, int64_t y_stride,
                                    float *grad_x, void *stream) {
	if (embed::freq_check("freq_encode_bwd", B, D, n_freq, C)) return 1;
	NR3D_CHECK(y_stride >= (int64_t)C, "freq_encode_bwd: y_stride = %lld is smaller than a row of %u", (long long)y_stride, C);
	if (B == 0) return 0;
	NR3D_CHECK(grad && y && grad_x, "freq_encode_bwd: NULL tensor pointer");
	const uint32_t total = (uint32_t)(B * D);
	hipLaunchKernelGGL(embed::k_freq_bwd, dim3(div_up(total, 256)), dim3(256), 0, (hipStream_t)stream, total, D, n_freq, C, grad, y, y_stride,
	                   grad_x);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_freq_encode_bwd_bwd(uint64_t B, uint32_t D, uint32_t n_freq, uint32_t C, const float *v, const float *grad, const float *y,
                                        int64_t y_stride, float *d_grad, float *d_x, void *stream) {
	if (embed::freq_check("freq_encode_bwd_bwd", B, D, n_freq, C)) return 1;
	NR3D_CHECK(y_stride >= (int64_t)C, "freq_encode_bwd_bwd: y_stride = %lld is smaller than a row of %u", (long long)y_stride, C);
	if (B == 0 || (!d_grad && !d_x)) return 0;
	NR3D_CHECK(v && y && (grad || !d_x), "freq_encode_bwd_bwd: NULL tensor pointer (grad may be NULL only without d_x)");
	hipStream_t st = (hipStream_t)stream;
	const uint32_t total = (uint32_t)(B * (d_grad ? C : D));
	const dim3 grid(div_up(total, 256)), block(256);
	if (d_grad && d_x) hipLaunchKernelGGL((embed::k_freq_bwd_bwd<true, true>), grid, block, 0, st, total, D, n_freq, C, v, grad, y, y_stride, d_grad, d_x);
	else if (d_grad) hipLaunchKernelGGL((embed::k_freq_bwd_bwd<true, false>), grid, block, 0, st, total, D, n_freq, C, v, grad, y, y_stride, d_grad, d_x);
	else hipLaunchKernelGGL((embed::k_freq_bwd_bwd<false, true>), grid, block, 0, st, total, D, n_freq, C, v, grad, y, y_stride, d_grad, d_x);
	NR3D_LAUNCH_CHECK();
	return 0;
}
