// nr3d_lib_amd/csrc/neus_upsample.hip -- one up-sampling stage of the NeuS ray queries in one launch: on the fixed-length rows of the
// vanilla coarse query (k_stage) and on the packs of the occupancy-march queries (k_stage_packed, further down; with LABELS the
// same body carries the block index of a forest's samples along).
//
// The reference runs a stage between two SDF queries as a chain of small torch ops (nr3d_lib/graphics/neus/neus_ray_query.py:258-270:
// neus_ray_sdf_to_alpha | neus_ray_sdf_to_upsample_alpha -> ray_alpha_to_vw -> batch_sample_pdf -> cat -> sort).  Rows hold tens to a
// few hundred floats, so launches and the sort dominate.  Here one 64-lane wave owns one ray, with the building blocks of wave_row.h:
// the row (depths, SDF, CDF, new depths) is staged in LDS.  No workspace; every output element is written exactly once by a fixed lane
// in a fixed order, so the result is the same bits run after run.
#include "common.h"
#include "wave_row.h"

namespace nr3d {
namespace neus_upsample {

using namespace wave_row;    // wave_sync() and its visibility argument, the scans, running_max, merge_slot

constexpr int kMaxRow = NR3D_NEUS_UPSAMPLE_MAX_ROW;   // cap on n + m: 3 n + m floats of LDS per wave stay below 12 KiB
constexpr int kWaves = 4;                              // rays per workgroup

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

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
		const float incl = incl_mul(1.0f - alpha, lane);
		float excl = __shfl_up(incl, 1, 64);
		if (lane == 0) excl = 1.0f;
		const float w = alpha * (carry_T * excl);
		carry_T *= __shfl(incl, 63, 64);
		total += __shfl(incl_add(w, lane), 63, 64);
		if (i < n) C[i] = w;
	}
	wave_sync();

	// ---- cdf_0 = 0, cdf_{i+1} = cdf_i + w_i / max(total, 1e-5), written over the weights at the same index ----
	const float norm = fmaxf(total, 1e-5f);
	float carry_c = 0.0f;
	for (int b = 0; b < n; b += 64) {
		const int i = b + lane;
		const float pdf = i < n ? C[i] / norm : 0.0f;
		const float incl = incl_add(pdf, lane);
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
		f = running_max(f, lane, carry_f);                    // the merge below needs a sorted row
		if (j < m) {
			F[j] = f;
			fine[(size_t)r * m + j] = f;
		}
	}
	wave_sync();

	// ---- the sorted union of D and F, depths first on ties ----
	const int nm = n + m;
	float *m_row = merged + (size_t)r * nm;
	int32_t *o_row = order + (size_t)r * nm;
	for (int p = lane; p < nm; p += 64) {
		const Slot s = merge_slot<true>(p, n, m, D, F);
		m_row[p] = s.from_a ? D[s.i] : F[s.j];
		o_row[p] = s.from_a ? s.i : n + s.j;
	}
}

// ---- the packed stage: the same scheme on the packs of a marcher (nr3d_neus_upsample_stage_packed) ----------------------------------
// One wave per pack, its length from pack_infos.  The arithmetic restates the packed op chain of the march-occ drivers
// (neus_packed_sdf_to_alpha | neus_packed_sdf_to_upsample_alpha -> packed_alpha_to_vw -> exclusive packed_cumsum -> packed_div ->
// packed_invert_cdf -> merge_two_packs_sorted_aligned), which is not the row chain above: the estimate's mid-point and half step are
// formed differently, the weights stop at a transmittance below 1e-4, the CDF is summed first and divided afterwards, the inversion
// returns the bin's lower depth for a pmf below 1e-5 and lerps with one fmaf, and the merge puts a new depth BEFORE an equal old one.
constexpr int kPackedLdsRow = NR3D_NEUS_UPSAMPLE_PACKED_LDS_ROW;   // packs with len + m up to this are staged: kWaves * 3 L floats of LDS

// The body over the pack's four arrays: D, S = depths and SDF [n], C = the CDF [n], F = the new depths [m].  Called once with LDS
// pointers and once with global ones; inlined, each call resolves to DS or global instructions.  Only this wave touches these rows, in
// both address spaces, which is what wave_sync() needs (wave_row.h).
//
// LABELS (nr3d_neus_upsample_stage_packed with blidx): every sample carries an int64 label, the forest's block index, that nothing here
// interprets.  A new depth takes the label of the inversion's `pos`, the upper end of its CDF bin, before the running maximum; the
// union carries the labels along.  Labels never enter LDS: `lb.in` is read once per new depth behind its binary search and once per
// old element in the merge, and a new element's label is read back from `lb.fine`, which this wave alone wrote before the
// wave_sync() in front of the merge -- the rule that lets the unstaged body read F from global memory.
template <bool LABELS> struct Labels {};
template <> struct Labels<true> {
	const int64_t *in;       // the pack's labels [n]
	int64_t *fine;           // [m], always written
	int64_t *merged;         // the pack's place in blidx_merged [n + m], read with merge only
};

template <bool ESTIMATE, bool STAGED, bool LABELS>
__device__ __forceinline__ void packed_body(int n, int m, int lane, const float *D, const float *S, float *C, float *F,
                                            const float *__restrict__ u_row, float inv_s, float *__restrict__ fine_row, bool merge,
                                            int64_t out_begin, float *__restrict__ m_row, float *__restrict__ s_row,
                                            int64_t *__restrict__ pidx_row, const Labels<LABELS> lb) {
	// ---- weights of the n - 1 intervals (w_{n-1} = 0) and, at the same index, their exclusive sum into C ----
	float carry_T = 1.0f, carry_c = 0.0f;
	bool stopped = false;
	for (int b = 0; b < n; b += 64) {
		const int i = b + lane;
		float alpha = 0.0f;
		if (i < n - 1) {
			const float s0 = S[i], s1 = S[i + 1];
			float c_prev, c_next;
			if (ESTIMATE) {
				const float d0 = D[i], delta = D[i + 1] - d0, d_sdf = s1 - s0;
				const float slope = d_sdf / (delta + 1e-5f);
				const float before = i > 0 ? (s0 - S[i - 1]) / ((d0 - D[i - 1]) + 1e-5f) : 0.0f;
				const float sl = fminf(fmaxf(fminf(before, slope), -10.0f), 0.0f);
				const float mid = s0 + d_sdf * 0.5f, half = sl * delta * 0.5f;
				c_prev = sigmoidf((mid - half) * inv_s);
				c_next = sigmoidf((mid + half) * inv_s);
			} else {
				c_prev = sigmoidf(s0 * inv_s);
				c_next = sigmoidf(s1 * inv_s);
			}
			alpha = fmaxf((c_prev - c_next) / (c_prev + 1e-5f), 0.0f);
		}
		// packed_alpha_to_vw(early_stop_eps = 1e-4, alpha_thre = 0): an alpha <= 0 leaves T as it is; w = alpha T while T >= 1e-4 and
		// 0 from the first T below on (decided on the scanned T: the product associates as a tree)
		const float incl = incl_mul(alpha <= 0.0f ? 1.0f : 1.0f - alpha, lane);
		float excl = __shfl_up(incl, 1, 64);
		if (lane == 0) excl = 1.0f;
		const float T = carry_T * excl;
		const unsigned long long below = __ballot(T < 1e-4f);
		const int first = below ? __ffsll((long long)below) - 1 : 64;
		const float w = (stopped || lane >= first) ? 0.0f : alpha * T;
		stopped = stopped || below != 0ull;
		carry_T *= __shfl(incl, 63, 64);
		const float incl_w = carry_c + incl_add(w, lane);
		const float before_w = __shfl_up(incl_w, 1, 64);
		if (i < n) C[i] = lane == 0 ? carry_c : before_w;
		carry_c = __shfl(incl_w, 63, 64);
	}
	wave_sync();

	// ---- cdf_i / max(cdf_{n-1}, 1e-5) ----
	const float norm = n > 0 ? fmaxf(C[n - 1], 1e-5f) : 1.0f;
	wave_sync();                                              // every lane holds cdf_{n-1} before its owner divides it
	for (int i = lane; i < n; i += 64) C[i] = C[i] / norm;
	wave_sync();

	// ---- inverse CDF at every u_j, raised to its running maximum: the merge needs a sorted row ----
	float carry_f = -INFINITY;
	for (int b = 0; b < m; b += 64) {
		const int j = b + lane;
		float f = -INFINITY;
		if (j < m) {
			f = 0.0f;                                         // a pack without elements (outside the contract) has nothing to read
			[[maybe_unused]] int64_t label = -1;
			if (n > 0) {
				// packed_invert_cdf's rule (k_invert_cdf, pack_ops.hip).  Written out on purpose: behind a shared function this kernel measured
				// 0.2 - 0.5 % slower at 65 536 packs, and nerf_upsample.hip's stage likewise (profiles/wave_row.md)
				const float uj = u_row[j];
				int lo = 0, hi = n;
				while (lo < hi) {
					const int mid = (lo + hi) >> 1;
					if (C[mid] < uj) lo = mid + 1; else hi = mid;
				}
				const int pos = min(lo, n - 1);
				if (pos == 0) f = D[0];
				else {
					const float c0 = C[pos - 1], pmf = C[pos] - c0, d0 = D[pos - 1];
					f = pmf < 1e-5f ? d0 : fmaf((uj - c0) / pmf, D[pos] - d0, d0);
				}
				if constexpr (LABELS) label = lb.in[pos];
			}
			if constexpr (LABELS) lb.fine[j] = label;
		}
		f = running_max(f, lane, carry_f);
		if (j < m) {
			F[j] = f;
			if (STAGED) fine_row[j] = f;
		}
	}
	if (!merge) return;
	wave_sync();

	// ---- the sorted union of D and F, a new depth before an equal old one ----
	const int nm = n + m;
	for (int q = lane; q < nm; q += 64) {
		const Slot s = merge_slot<false>(q, n, m, D, F);
		m_row[q] = s.from_a ? D[s.i] : F[s.j];
		if (!s.from_a) pidx_row[s.j] = out_begin + q;
		else if (s_row) s_row[q] = S[s.i];
		if constexpr (LABELS) lb.merged[q] = s.from_a ? lb.in[s.i] : lb.fine[s.j];
	}
}

template <bool ESTIMATE, bool LABELS>
__global__ __launch_bounds__(kWaves * 64) void k_stage_packed(uint32_t P, int64_t N, int m, const float *__restrict__ depth,
                                                               const float *__restrict__ sdf, const int64_t *__restrict__ pack_infos,
                                                               const float *__restrict__ u, int64_t u_stride, float inv_s,
                                                               float *__restrict__ cdf_ws, float *__restrict__ fine,
                                                               float *__restrict__ merged, float *__restrict__ sdf_merged,
                                                               int64_t *__restrict__ pidx_fine, int64_t *__restrict__ pack_infos_out,
                                                               const Labels<LABELS> labels) {
	__shared__ __attribute__((aligned(16))) float lds[kWaves * 3 * kPackedLdsRow];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t p = blockIdx.x * kWaves + wave;
	if (p >= P) return;                                   // wave-uniform; nothing below synchronises across waves
	// the pack, clipped to [0, N): whatever pack_infos holds, every access below stays inside the buffers
	// (these three lines stay written out for the same reason as the inverse CDF of packed_body)
	const int64_t b64 = pack_infos[2 * (size_t)p], n64 = pack_infos[2 * (size_t)p + 1];
	const int64_t first = b64 < 0 ? 0 : (b64 > N ? N : b64);
	const int n = (int)(n64 < 0 ? 0 : (n64 > N - first ? N - first : n64));
	const int64_t out_begin = first + (int64_t)p * m;
	const float *d_row = depth + first, *s_row = sdf + first, *u_row = u + (int64_t)p * u_stride;
	float *f_row = fine + (size_t)p * m;
	const bool merge = merged != nullptr;
	float *mo = merge ? merged + out_begin : nullptr, *so = sdf_merged ? sdf_merged + out_begin : nullptr;
	int64_t *po = merge ? pidx_fine + (size_t)p * m : nullptr;
	if (merge && lane == 0) {
		pack_infos_out[2 * (size_t)p] = out_begin;
		pack_infos_out[2 * (size_t)p + 1] = (int64_t)n + m;
	}
	Labels<LABELS> lb;
	if constexpr (LABELS) lb = {labels.in + first, labels.fine + (size_t)p * m, merge ? labels.merged + out_begin : nullptr};
	if (n + m <= kPackedLdsRow) {                         // wave-uniform
		float *D = lds + (size_t)wave * (3 * kPackedLdsRow), *S = D + n, *C = S + n, *F = C + n;
		for (int i = lane; i < n; i += 64) {
			D[i] = d_row[i];
			S[i] = s_row[i];
		}
		wave_sync();
		packed_body<ESTIMATE, true, LABELS>(n, m, lane, D, S, C, F, u_row, inv_s, f_row, merge, out_begin, mo, so, po, lb);
	} else {
		packed_body<ESTIMATE, false, LABELS>(n, m, lane, d_row, s_row, cdf_ws + first, f_row, u_row, inv_s, nullptr, merge, out_begin, mo, so,
		                                     po, lb);
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

extern "C" int nr3d_neus_upsample_packed_lds_row(void) { return neus_upsample::kPackedLdsRow; }

// LABELS picks the instantiation; `labels` is the kernel argument as the entry filled it
template <bool LABELS>
static void launch_stage_packed(uint32_t P, uint64_t N, uint32_t m, const float *depth, const float *sdf, const int64_t *pack_infos,
                                const float *u, int64_t u_stride, float inv_s, int use_estimate, float *cdf_workspace, float *fine,
                                float *merged, float *sdf_merged, int64_t *pidx_fine, int64_t *pack_infos_out,
                                const neus_upsample::Labels<LABELS> labels, hipStream_t st) {
	const dim3 grid(div_up(P, neus_upsample::kWaves)), block(neus_upsample::kWaves * 64);
	if (use_estimate)
		hipLaunchKernelGGL((neus_upsample::k_stage_packed<true, LABELS>), grid, block, 0, st, P, (int64_t)N, (int)m, depth, sdf, pack_infos, u,
		                   u_stride, inv_s, cdf_workspace, fine, merged, sdf_merged, pidx_fine, pack_infos_out, labels);
	else
		hipLaunchKernelGGL((neus_upsample::k_stage_packed<false, LABELS>), grid, block, 0, st, P, (int64_t)N, (int)m, depth, sdf, pack_infos, u,
		                   u_stride, inv_s, cdf_workspace, fine, merged, sdf_merged, pidx_fine, pack_infos_out, labels);
}

extern "C" int nr3d_neus_upsample_stage_packed(uint32_t P, uint64_t N, uint32_t m, const float *depth, const float *sdf,
                                               const int64_t *blidx, const int64_t *pack_infos, const float *u, int64_t u_stride,
                                               float inv_s, int use_estimate, int merge, int need_sdf, float *cdf_workspace, float *fine,
                                               int64_t *blidx_fine, float *merged, float *sdf_merged, int64_t *blidx_merged,
                                               int64_t *pidx_fine, int64_t *pack_infos_out, void *stream) {
	NR3D_CHECK(m >= 1, "neus_upsample_stage_packed: m = %u, at least 1 new depth per pack", m);
	NR3D_CHECK(u_stride == 0 || u_stride == (int64_t)m, "neus_upsample_stage_packed: u_stride = %lld, must be 0 (one shared row) or m = %u",
	           (long long)u_stride, m);
	NR3D_CHECK(N < (1ull << 31) && N + (uint64_t)P * m < (1ull << 31),
	           "neus_upsample_stage_packed: N + P m = %llu + %u * %u, the merged buffer holds at most 2^31 - 1 elements",
	           (unsigned long long)N, P, m);
	NR3D_CHECK(!need_sdf || merge, "neus_upsample_stage_packed: need_sdf without merge");
	NR3D_CHECK(!blidx || blidx_fine, "neus_upsample_stage_packed: blidx without blidx_fine");
	NR3D_CHECK(blidx || (!blidx_fine && !blidx_merged), "neus_upsample_stage_packed: blidx_fine or blidx_merged without blidx");
	NR3D_CHECK(!(merge && blidx) || blidx_merged, "neus_upsample_stage_packed: merge with blidx but without blidx_merged");
	if (P == 0) return 0;
	NR3D_CHECK(depth && sdf && pack_infos && u && cdf_workspace && fine, "neus_upsample_stage_packed: NULL tensor pointer");
	NR3D_CHECK(!merge || (merged && pidx_fine && pack_infos_out),
	           "neus_upsample_stage_packed: merge without merged, pidx_fine or pack_infos_out");
	NR3D_CHECK(!need_sdf || sdf_merged, "neus_upsample_stage_packed: need_sdf without sdf_merged");
	float *mg = merge ? merged : nullptr, *sm = need_sdf ? sdf_merged : nullptr;
	if (!blidx)   // (named first: the kernels stand in the code object in the order they are instantiated in)
		launch_stage_packed<false>(P, N, m, depth, sdf, pack_infos, u, u_stride, inv_s, use_estimate, cdf_workspace, fine, mg, sm, pidx_fine,
		                           pack_infos_out, {}, (hipStream_t)stream);
	else
		launch_stage_packed<true>(P, N, m, depth, sdf, pack_infos, u, u_stride, inv_s, use_estimate, cdf_workspace, fine, mg, sm, pidx_fine,
		                          pack_infos_out, {blidx, blidx_fine, merge ? blidx_merged : nullptr}, (hipStream_t)stream);
	NR3D_LAUNCH_CHECK();
	return 0;
}
