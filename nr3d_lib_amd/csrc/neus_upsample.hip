// nr3d_lib_amd/csrc/neus_upsample.hip -- one up-sampling stage of the vanilla NeuS coarse ray query on fixed-length rows, in one launch.
//
// The reference runs a stage between two SDF queries as a chain of small torch ops (nr3d_lib/graphics/neus/neus_ray_query.py:258-270:
// neus_ray_sdf_to_alpha | neus_ray_sdf_to_upsample_alpha -> ray_alpha_to_vw -> batch_sample_pdf -> cat -> sort).  Rows hold tens to a
// few hundred floats, so launches and the sort dominate.  Here one 64-lane wave owns one ray: the row (depths, SDF, CDF, new depths)
// is staged in LDS, products and sums are wave scans over 64-element chunks with a carry, the inverse CDF is a binary search in LDS,
// and -- both lists being sorted -- the merge is a merge-path search per output slot instead of a sort.  No atomics, no workspace;
// every output element is written exactly once by a fixed lane in a fixed order, so the result is the same bits run after run.
#include "common.h"

namespace nr3d {
namespace neus_upsample {

constexpr int kMaxRow = NR3D_NEUS_UPSAMPLE_MAX_ROW;   // cap on n + m: 3 n + m floats of LDS per wave stay below 12 KiB
constexpr int kWaves = 4;                              // rays per workgroup

// LDS written by some lanes of the wave is read by others: order the DS traffic of the wave (no other wave shares these rows)
__device__ __forceinline__ void wave_sync() {
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float wave_incl_mul(float v, int lane) {
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const float t = __shfl_up(v, off, 64);
		if (lane >= off) v *= t;
	}
	return v;
}
__device__ __forceinline__ float wave_incl_add(float v, int lane) {
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const float t = __shfl_up(v, off, 64);
		if (lane >= off) v += t;
	}
	return v;
}
__device__ __forceinline__ float wave_incl_max(float v, int lane) {
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const float t = __shfl_up(v, off, 64);
		if (lane >= off) v = fmaxf(v, t);
	}
	return v;
}

template <bool ESTIMATE>
__global__ __launch_bounds__(kWaves * 64) void k_stage(uint32_t R, int n, int m, const float *__restrict__ depth,
                                                        const float *__restrict__ sdf, const float *__restrict__ u, int64_t u_stride,
                                                        float inv_s, float *__restrict__ fine, float *__restrict__ merged,
                                                        int32_t *__restrict__ order) {
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * kWaves + wave;
	if (r >= R) return;                                   // wave-uniform; nothing below synchronises across waves
	float *D = lds + (size_t)wave * (3 * n + m), *S = D + n, *C = S + n, *F = C + n;
	const float *d_row = depth + (size_t)r * n, *s_row = sdf + (size_t)r * n, *u_row = u + (int64_t)r * u_stride;

	for (int i = lane; i < n; i += 64) {
		D[i] = d_row[i];
		S[i] = s_row[i];
	}
	wave_sync();

	// ---- weights of the n - 1 intervals into C[0 .. n-1) (C[n-1] = 0), their sum in `total` ----
	float carry_T = 1.0f, total = 0.0f;
	for (int b = 0; b < n; b += 64) {
		const int i = b + lane;
		float alpha = 0.0f;
		if (i < n - 1) {
			const float s0 = S[i], s1 = S[i + 1];
			float c_prev, c_next;
			if (ESTIMATE) {
				const float d0 = D[i], delta = D[i + 1] - d0;
				const float slope = (s1 - s0) / (delta + 1e-5f);
				const float before = i > 0 ? (s0 - S[i - 1]) / ((d0 - D[i - 1]) + 1e-5f) : 0.0f;
				const float sl = fminf(fmaxf(fminf(before, slope), -10.0f), 0.0f);
				const float mid = (s0 + s1) * 0.5f;
				c_prev = sigmoidf((mid + sl * (delta * -0.5f)) * inv_s);
				c_next = sigmoidf((mid + sl * (delta * 0.5f)) * inv_s);
			} else {
				c_prev = sigmoidf(s0 * inv_s);
				c_next = sigmoidf(s1 * inv_s);
			}
			alpha = fmaxf((c_prev - c_next) / (c_prev + 1e-5f), 0.0f);
		}
		// (1 + 1e-10) - alpha in fp32 is 1 - alpha; lanes past the row multiply by 1
		const float incl = wave_incl_mul(1.0f - alpha, lane);
		float excl = __shfl_up(incl, 1, 64);
		if (lane == 0) excl = 1.0f;
		const float w = alpha * (carry_T * excl);
		carry_T *= __shfl(incl, 63, 64);
		total += __shfl(wave_incl_add(w, lane), 63, 64);
		if (i < n) C[i] = w;
	}
	wave_sync();

	// ---- cdf_0 = 0, cdf_{i+1} = cdf_i + w_i / max(total, 1e-5), written over the weights at the same index ----
	const float norm = fmaxf(total, 1e-5f);
	float carry_c = 0.0f;
	for (int b = 0; b < n; b += 64) {
		const int i = b + lane;
		const float pdf = i < n ? C[i] / norm : 0.0f;
		const float incl = wave_incl_add(pdf, lane);
		float before = __shfl_up(incl, 1, 64);
		if (i < n) C[i] = lane == 0 ? carry_c : carry_c + before;      // the inclusive sum up to interval i - 1
		carry_c += __shfl(incl, 63, 64);
	}
	wave_sync();

	// ---- inverse CDF at every u_j ----
	float carry_f = -INFINITY;
	for (int b = 0; b < m; b += 64) {
		const int j = b + lane;
		float f = -INFINITY;
		if (j < m) {
			const float uj = u_row[j];
			int lo = 0, hi = n;                               // first k with C[k] >= uj, n when there is none
			while (lo < hi) {
				const int mid = (lo + hi) >> 1;
				if (C[mid] < uj) lo = mid + 1; else hi = mid;
			}
			const int below = max(lo - 1, 0), above = min(lo, n - 1);
			const float c0 = C[below], d0 = D[below];
			float den = C[above] - c0;
			if (den < 1e-5f) den = 1.0f;
			f = d0 + (uj - c0) / den * (D[above] - d0);
		}
		// d0 + t (d1 - d0) with t <= 1 can round one ulp above d1, where the next interval's samples start: a running maximum keeps the
		// row non-decreasing, which the merge below relies on (it changes nothing wherever the formula is monotone already)
		f = fmaxf(wave_incl_max(f, lane), carry_f);
		carry_f = __shfl(f, 63, 64);
		if (j < m) {
			F[j] = f;
			fine[(size_t)r * m + j] = f;
		}
	}
	wave_sync();

	// ---- merge path: output slot p takes D[i] or F[p - i], i = the number of depths among the first p outputs (depths first on ties);
	// every index below is in range by construction of the search interval, whatever the values are ----
	const int nm = n + m;
	float *m_row = merged + (size_t)r * nm;
	int32_t *o_row = order + (size_t)r * nm;
	for (int p = lane; p < nm; p += 64) {
		int lo = max(0, p - m), hi = min(p, n);
		while (lo < hi) {
			const int mid = (lo + hi) >> 1;                    // lo <= mid < hi: mid < n, 1 <= p - mid <= m
			if (D[mid] <= F[p - mid - 1]) lo = mid + 1; else hi = mid;
		}
		const int i = lo, j = p - lo;
		const bool from_depth = i < n && (j >= m || D[i] <= F[j]);
		m_row[p] = from_depth ? D[i] : F[j];
		o_row[p] = from_depth ? i : n + j;
	}
}

}  // namespace neus_upsample
}  // namespace nr3d

using namespace nr3d;

extern "C" int nr3d_neus_upsample_max_row(void) { return neus_upsample::kMaxRow; }

extern "C" int nr3d_neus_upsample_stage(uint32_t R, uint32_t n, uint32_t m, const float *depth, const float *sdf, const float *u,
                                        int64_t u_stride, float inv_s, int use_estimate, float *fine, float *merged, int32_t *order,
                                        void *stream) {
	NR3D_CHECK(n >= 2, "neus_upsample_stage: n = %u, a row needs at least 2 boundaries", n);
	NR3D_CHECK(m >= 1, "neus_upsample_stage: m = %u, at least 1 new depth per row", m);
	NR3D_CHECK((uint64_t)n + m <= (uint64_t)neus_upsample::kMaxRow, "neus_upsample_stage: n + m = %llu, rows of at most %d are served",
	           (unsigned long long)((uint64_t)n + m), neus_upsample::kMaxRow);
	NR3D_CHECK(u_stride == 0 || u_stride == (int64_t)m, "neus_upsample_stage: u_stride = %lld, must be 0 (one shared row) or m = %u",
	           (long long)u_stride, m);
	NR3D_CHECK(R < (1u << 31), "neus_upsample_stage: R = %u, at most 2^31 - 1 rays per call", R);
	if (R == 0) return 0;
	NR3D_CHECK(depth && sdf && u && fine && merged && order, "neus_upsample_stage: NULL tensor pointer");
	const dim3 grid(div_up(R, neus_upsample::kWaves)), block(neus_upsample::kWaves * 64);
	const size_t lds = (size_t)neus_upsample::kWaves * (3 * (size_t)n + m) * sizeof(float);     // < 48 KiB at the cap
	hipStream_t st = (hipStream_t)stream;
	if (use_estimate)
		hipLaunchKernelGGL(neus_upsample::k_stage<true>, grid, block, lds, st, R, (int)n, (int)m, depth, sdf, u, u_stride, inv_s, fine,
		                   merged, order);
	else
		hipLaunchKernelGGL(neus_upsample::k_stage<false>, grid, block, lds, st, R, (int)n, (int)m, depth, sdf, u, u_stride, inv_s, fine,
		                   merged, order);
	NR3D_LAUNCH_CHECK();
	return 0;
}
