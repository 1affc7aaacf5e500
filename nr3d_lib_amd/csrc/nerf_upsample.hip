// nr3d_lib_amd/csrc/nerf_upsample.hip -- the packed stages of the NeRF march + up-sample ray query in one launch each: the union of
// the coarse rows with the marched packs (k_merge_rows_packs) and one importance-resampling stage on the density (k_nerf_stage_packed).
//
// The reference runs both between two density queries as chains of small torch ops (nr3d_lib/graphics/nerf/nerf_ray_query.py:289-302:
// merge_two_packs_sorted_a_includes_b, four index-puts, addcmul, packed_diff; :332-360: tau_to_alpha, packed_cumsum, a gather,
// packed_div, packed_sample_cdf, a second merge with its sort, four more index-puts, packed_diff) on packs of a few dozen to a few
// hundred floats.  Here one 64-lane wave owns one ray or pack, with the building blocks of wave_row.h; short rows are staged in LDS,
// longer ones stay in global memory.  No host wait; every output element is written exactly once by a fixed lane in a fixed order, so
// the result is the same bits run after run.
#include "common.h"
#include "wave_row.h"

namespace nr3d {
namespace nerf_upsample {

constexpr int kLdsRow = NR3D_NERF_UPSAMPLE_LDS_ROW;    // rows up to this are staged: kWaves * 2 L floats of LDS per workgroup, both kernels
constexpr int kWaves = 4;                              // rays or packs per workgroup

using namespace wave_row;    // wave_sync() and its visibility argument, the scans, running_max, merge_value (B first on ties)

// ---- (a) coarse rows U marched packs -------------------------------------------------------------------------------------------------
// A = the ray's coarse row [nc], B = its marched pack [n], M = the union [nc + n]: LDS rows (STAGED, then d_out receives a copy) or the
// global ones (then M is d_out itself and the differences read back what this wave stored).
template <bool STAGED>
__device__ __forceinline__ void merge_body(int nc, int n, int lane, const float *A, const float *B, float *M, int64_t r, float ox, float oy,
                                           float oz, float dx, float dy, float dz, float *__restrict__ d_out, float *__restrict__ dl_out,
                                           int64_t *__restrict__ r_out, float *__restrict__ x_out) {
	const int nm = nc + n;
	for (int q = lane; q < nm; q += 64) {
		const float t = merge_value<false>(q, nc, n, A, B);      // a marched depth before an equal coarse one
		M[q] = t;
		if (STAGED) d_out[q] = t;
		r_out[q] = r;
		// torch.addcmul(o, d, t) rounds the product before it adds (o + 1 * (d * t): its fma takes the scale, not d * t)
		x_out[3 * (size_t)q + 0] = __fadd_rn(ox, __fmul_rn(dx, t));
		x_out[3 * (size_t)q + 1] = __fadd_rn(oy, __fmul_rn(dy, t));
		x_out[3 * (size_t)q + 2] = __fadd_rn(oz, __fmul_rn(dz, t));
	}
	wave_sync();
	for (int q = lane; q < nm; q += 64) dl_out[q] = q + 1 < nm ? M[q + 1] - M[q] : 0.0f;
}

__global__ __launch_bounds__(kWaves * 64) void k_merge_rows_packs(uint32_t R, int nc, int64_t N, const float *__restrict__ coarse,
                                                                   const float *__restrict__ depth, const int64_t *__restrict__ pack_infos,
                                                                   const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                                   float *__restrict__ depths_all, float *__restrict__ deltas_all,
                                                                   int64_t *__restrict__ ridx_all, float *__restrict__ samples_all,
                                                                   int64_t *__restrict__ pack_infos_out) {
	__shared__ __attribute__((aligned(16))) float lds[kWaves * 2 * kLdsRow];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * kWaves + wave;
	if (r >= R) return;                                   // wave-uniform; nothing below synchronises across waves
	// the marched pack, clipped to [0, N): whatever pack_infos holds, every access below stays inside the buffers
	const int64_t b64 = pack_infos[2 * (size_t)r], n64 = pack_infos[2 * (size_t)r + 1];
	const int64_t first = b64 < 0 ? 0 : (b64 > N ? N : b64);
	const int n = (int)(n64 < 0 ? 0 : (n64 > N - first ? N - first : n64));
	const int64_t out_begin = (int64_t)r * nc + first;
	if (lane == 0) {
		pack_infos_out[2 * (size_t)r] = out_begin;
		pack_infos_out[2 * (size_t)r + 1] = (int64_t)nc + n;
	}
	const float *a_row = coarse + (size_t)r * nc, *b_row = depth + first;
	const float *o = rays_o + 3 * (size_t)r, *d = rays_d + 3 * (size_t)r;
	const float ox = o[0], oy = o[1], oz = o[2], dx = d[0], dy = d[1], dz = d[2];
	float *d_out = depths_all + out_begin, *dl_out = deltas_all + out_begin, *x_out = samples_all + 3 * out_begin;
	int64_t *r_out = ridx_all + out_begin;
	if ((int64_t)nc + n <= kLdsRow) {                     // wave-uniform
		float *A = lds + (size_t)wave * (2 * kLdsRow), *B = A + nc, *M = B + n;
		for (int i = lane; i < nc; i += 64) A[i] = a_row[i];
		for (int i = lane; i < n; i += 64) B[i] = b_row[i];
		wave_sync();
		merge_body<true>(nc, n, lane, A, B, M, (int64_t)r, ox, oy, oz, dx, dy, dz, d_out, dl_out, r_out, x_out);
	} else {
		merge_body<false>(nc, n, lane, a_row, b_row, d_out, (int64_t)r, ox, oy, oz, dx, dy, dz, d_out, dl_out, r_out, x_out);
	}
}

// ---- (b) one up-sampling stage on the density ---------------------------------------------------------------------------------------
// The body over the pack's arrays: D = depths [n], C = the CDF [n], F = the new depths [m], K = the coarse row [nc], M = the union
// [nc + m].  Called once with LDS pointers (STAGED: fine_row, m_row receive copies) and once with global ones (C in the caller's
// workspace, F and M the output rows themselves); inlined, each call resolves to DS or global instructions.
template <bool STAGED>
__device__ __forceinline__ void stage_body(int n, int m, int nc, int lane, const float *D, const float *__restrict__ sigma,
                                           const float *__restrict__ delta, float *C, float *F, const float *K, float *M,
                                           const float *__restrict__ u_row, float *__restrict__ fine_row, float *__restrict__ m_row,
                                           float *__restrict__ dl_row) {
	// ---- alpha_i = 1 - exp(-sigma_i delta_i) and its inclusive sum into C; the pack's sum stays in `carry` on every lane.  The opacity
	// is evaluated as -expm1(-sigma delta): the same quantity without the cancellation that leaves 1 - exp(-x) a multiple of 2^-24
	// for a small optical depth x, which is where the CDF is flat and its inverse steep ----
	float carry = 0.0f;
	for (int b = 0; b < n; b += 64) {
		const int i = b + lane;
		const float alpha = i < n ? -expm1f(-(sigma[i] * delta[i])) : 0.0f;
		const float incl = carry + incl_add(alpha, lane);
		if (i < n) C[i] = incl;
		carry = __shfl(incl, 63, 64);
	}
	// ---- cdf_i = c_i / max(c_{n-1}, 1e-5): every lane divides what it stored itself ----
	const float norm = fmaxf(carry, 1e-5f);
	for (int i = lane; i < n; i += 64) C[i] = C[i] / norm;
	wave_sync();

	// ---- inverse CDF at every u_j (k_invert_cdf, pack_ops.hip), raised to its running maximum: the union below needs a sorted row (the
	// reference sorts it) ----
	float carry_f = -INFINITY;
	for (int b = 0; b < m; b += 64) {
		const int j = b + lane;
		float f = -INFINITY;
		if (j < m) {
			f = 0.0f;                                         // a pack without elements (outside the contract) has nothing to read
			if (n > 0) {
				const float uj = u_row[j];
				int lo = 0, hi = n;                           // first k with C[k] >= uj, n when there is none
				while (lo < hi) {
					const int mid = (lo + hi) >> 1;
					if (C[mid] < uj) lo = mid + 1; else hi = mid;
				}
				const int pos = min(lo, n - 1);
				if (pos == 0) f = D[0];
				else {
					const float c0 = C[pos - 1], pmf = C[pos] - c0, d0 = D[pos - 1];
					f = pmf < 1e-5f ? d0 : __fmaf_rn((uj - c0) / pmf, D[pos] - d0, d0);
				}
			}
		}
		f = running_max(f, lane, carry_f);
		if (j < m) {
			F[j] = f;
			if (STAGED) fine_row[j] = f;
		}
	}
	wave_sync();

	if (nc == 0) {
		// ---- no coarse row: deltas_j = fine_{j+1} - fine_j, depths_j = fine_j + deltas_j (the whole difference, as the reference adds) ----
		for (int j = lane; j < m - 1; j += 64) {
			const float f0 = F[j], df = F[j + 1] - f0;
			dl_row[j] = df;
			m_row[j] = f0 + df;
		}
		return;
	}
	// ---- the sorted union of the coarse row and the new depths, then its differences ----
	const int nm = nc + m;
	for (int q = lane; q < nm; q += 64) {
		const float t = merge_value<false>(q, nc, m, K, F);       // a new depth before an equal coarse one
		M[q] = t;
		if (STAGED) m_row[q] = t;
	}
	wave_sync();
	for (int q = lane; q < nm; q += 64) dl_row[q] = q + 1 < nm ? M[q + 1] - M[q] : 0.0f;
}

__global__ __launch_bounds__(kWaves * 64) void k_nerf_stage_packed(uint32_t P, int64_t N, int m, int nc, int64_t n_coarse_rows,
                                                                    const float *__restrict__ depth, const float *__restrict__ sigma,
                                                                    const float *__restrict__ delta, const int64_t *__restrict__ pack_infos,
                                                                    const float *__restrict__ u, int64_t u_stride,
                                                                    const float *__restrict__ coarse, const int64_t *__restrict__ coarse_row,
                                                                    float *__restrict__ cdf_ws, float *__restrict__ fine,
                                                                    float *__restrict__ merged, float *__restrict__ deltas) {
	__shared__ __attribute__((aligned(16))) float lds[kWaves * 2 * kLdsRow];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t p = blockIdx.x * kWaves + wave;
	if (p >= P) return;                                   // wave-uniform; nothing below synchronises across waves
	// the pack, clipped to [0, N), and its coarse row, clipped to the rows there are: no access below leaves the buffers
	const int64_t b64 = pack_infos[2 * (size_t)p], n64 = pack_infos[2 * (size_t)p + 1];
	const int64_t first = b64 < 0 ? 0 : (b64 > N ? N : b64);
	const int n = (int)(n64 < 0 ? 0 : (n64 > N - first ? N - first : n64));
	const float *k_row = nullptr;
	if (nc > 0) {
		int64_t row = coarse_row ? coarse_row[p] : (int64_t)p;
		row = row < 0 ? 0 : (row >= n_coarse_rows ? n_coarse_rows - 1 : row);
		k_row = coarse + (size_t)row * nc;
	}
	const int width = nc > 0 ? nc + m : m - 1;            // of merged / deltas
	const float *d_row = depth + first, *u_row = u + (int64_t)p * u_stride;
	float *f_row = fine + (size_t)p * m, *m_row = merged + (size_t)p * width, *dl_row = deltas + (size_t)p * width;
	if ((int64_t)n + m + nc <= kLdsRow) {                 // wave-uniform
		float *D = lds + (size_t)wave * (2 * kLdsRow), *C = D + n, *F = C + n, *K = F + m, *M = K + nc;
		for (int i = lane; i < n; i += 64) D[i] = d_row[i];
		for (int i = lane; i < nc; i += 64) K[i] = k_row[i];
		wave_sync();
		stage_body<true>(n, m, nc, lane, D, sigma + first, delta + first, C, F, K, M, u_row, f_row, m_row, dl_row);
	} else {
		stage_body<false>(n, m, nc, lane, d_row, sigma + first, delta + first, cdf_ws + first, f_row, k_row, m_row, u_row, nullptr, m_row,
		                  dl_row);
	}
}

}  // namespace nerf_upsample
}  // namespace nr3d

using namespace nr3d;

extern "C" int nr3d_nerf_upsample_lds_row(void) { return nerf_upsample::kLdsRow; }

extern "C" int nr3d_nerf_merge_rows_packs(uint32_t R, uint32_t num_coarse, uint64_t N, const float *coarse, const float *depth,
                                          const int64_t *pack_infos_all, const float *rays_o, const float *rays_d, float *depths_all,
                                          float *deltas_all, int64_t *ridx_all, float *samples_all, int64_t *pack_infos_out, void *stream) {
	NR3D_CHECK(num_coarse >= 1, "nerf_merge_rows_packs: num_coarse = %u, at least 1 coarse depth per ray", num_coarse);
	NR3D_CHECK(N < (1ull << 31) && N + (uint64_t)R * num_coarse < (1ull << 31),
	           "nerf_merge_rows_packs: N + R num_coarse = %llu + %u * %u, the merged buffer holds at most 2^31 - 1 elements",
	           (unsigned long long)N, R, num_coarse);
	if (R == 0) return 0;
	NR3D_CHECK(coarse && pack_infos_all && rays_o && rays_d && depths_all && deltas_all && ridx_all && samples_all && pack_infos_out,
	           "nerf_merge_rows_packs: NULL tensor pointer");
	NR3D_CHECK(depth || N == 0, "nerf_merge_rows_packs: NULL depth with N = %llu", (unsigned long long)N);
	const dim3 grid(div_up(R, nerf_upsample::kWaves)), block(nerf_upsample::kWaves * 64);
	hipLaunchKernelGGL(nerf_upsample::k_merge_rows_packs, grid, block, 0, (hipStream_t)stream, R, (int)num_coarse, (int64_t)N, coarse, depth,
	                   pack_infos_all, rays_o, rays_d, depths_all, deltas_all, ridx_all, samples_all, pack_infos_out);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_nerf_upsample_stage_packed(uint32_t P, uint64_t N, uint32_t m, uint32_t num_coarse, uint64_t n_coarse_rows,
                                               const float *depth, const float *sigma, const float *delta, const int64_t *pack_infos,
                                               const float *u, int64_t u_stride, const float *coarse, const int64_t *coarse_row,
                                               float *cdf_workspace, float *fine, float *merged, float *deltas, void *stream) {
	NR3D_CHECK(m >= 1, "nerf_upsample_stage_packed: m = %u, at least 1 new depth per pack", m);
	NR3D_CHECK(u_stride == 0 || u_stride == (int64_t)m, "nerf_upsample_stage_packed: u_stride = %lld, must be 0 (one shared row) or m = %u",
	           (long long)u_stride, m);
	NR3D_CHECK(N < (1ull << 31) && (uint64_t)P * ((uint64_t)m + num_coarse) < (1ull << 31) && m < (1u << 30) && num_coarse < (1u << 30),
	           "nerf_upsample_stage_packed: N = %llu, P (m + num_coarse) = %u * (%u + %u): at most 2^31 - 1 elements each",
	           (unsigned long long)N, P, m, num_coarse);
	NR3D_CHECK(num_coarse == 0 || n_coarse_rows >= 1, "nerf_upsample_stage_packed: num_coarse = %u without a coarse row", num_coarse);
	if (P == 0) return 0;
	NR3D_CHECK(depth && sigma && delta && pack_infos && u && cdf_workspace && fine, "nerf_upsample_stage_packed: NULL tensor pointer");
	NR3D_CHECK(num_coarse == 0 || coarse, "nerf_upsample_stage_packed: num_coarse = %u with NULL coarse", num_coarse);
	NR3D_CHECK((merged && deltas) || (num_coarse == 0 && m == 1), "nerf_upsample_stage_packed: NULL merged or deltas");
	const dim3 grid(div_up(P, nerf_upsample::kWaves)), block(nerf_upsample::kWaves * 64);
	hipLaunchKernelGGL(nerf_upsample::k_nerf_stage_packed, grid, block, 0, (hipStream_t)stream, P, (int64_t)N, (int)m, (int)num_coarse,
	                   (int64_t)n_coarse_rows, depth, sigma, delta, pack_infos, u, u_stride, coarse, coarse_row, cdf_workspace, fine, merged,
	                   deltas);
	NR3D_LAUNCH_CHECK();
	return 0;
}
