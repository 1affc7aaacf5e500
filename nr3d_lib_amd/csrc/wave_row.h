// nr3d_lib_amd/csrc/wave_row.h -- the building blocks of the ray-stage kernels, in which one 64-lane wave owns one ray or pack
// (neus_upsample.hip, nerf_upsample.hip, neus_composite.hip, the prefix-product composite of pack_ops.hip): the wave's row lives in LDS
// or in global memory that no other wave touches, sums / products / maxima are shuffle scans over 64-element chunks with a carry, and
// the union of two sorted lists is a merge-path search per output slot instead of a sort.  No atomics, no workgroup barrier; every
// output element has one writer.  A new kernel of this family starts from here.
// NOT here, on purpose: the packed inverse CDF (k_invert_cdf of pack_ops.hip is its statement; the two packed stages keep it written
// out) and the three lines that clip a pack to [0, N).  Behind a function both cost the packed stages 0.2 - 0.6 % (profiles/wave_row.md).
#pragma once
#include "common.h"

namespace nr3d {
namespace wave_row {

// What some lanes of the wave store, other lanes of the SAME wave read back after wave_sync(); no other wave, workgroup or atomic
// shares these rows.  For LDS rows that orders the wave's DS traffic.  It is enough for rows in GLOBAL memory too: a wave's vector
// memory instructions reach its compute unit's L1 in program order, the L1 is write-through and nothing else writes these rows, so a
// load issued after a store of the same wave returns the stored value.  The wavefront-scope fence keeps the compiler from moving the
// accesses across it; no wider scope is needed because nothing outside the wave is involved.  A row that a second wave writes needs
// more than this.
__device__ __forceinline__ void wave_sync() {
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// Inclusive Kogge-Stone scans over the G neighbouring lanes a row occupies (G a power of two, gl = the lane's index in its group):
// log2 G shuffle steps; the operands associate as a tree, not left to right.  Every lane of the wave must call them.
template <int G = 64> __device__ __forceinline__ float incl_add(float v, int gl) {
#pragma unroll
	for (int off = 1; off < G; off <<= 1) { const float t = __shfl_up(v, off, G); if (gl >= off) v += t; }
	return v;
}
template <int G = 64> __device__ __forceinline__ float incl_mul(float v, int gl) {
#pragma unroll
	for (int off = 1; off < G; off <<= 1) { const float t = __shfl_up(v, off, G); if (gl >= off) v *= t; }
	return v;
}
template <int G = 64> __device__ __forceinline__ float incl_max(float v, int gl) {
#pragma unroll
	for (int off = 1; off < G; off <<= 1) { const float t = __shfl_up(v, off, G); if (gl >= off) v = fmaxf(v, t); }
	return v;
}

// One 64-element chunk of a row raised to its running maximum; `carry` (-INFINITY before the first chunk) holds the maximum so far on
// every lane, lanes past the row pass -INFINITY.  An inverse CDF d0 + t (d1 - d0) with t <= 1 can round one ulp above d1, where the
// next bin's samples start; merge_slot needs a sorted list.  Safe because the maximum changes nothing wherever the values are
// non-decreasing already, and where they are not it repeats the larger of two values an ulp apart (a sort would swap them).
__device__ __forceinline__ float running_max(float f, int lane, float &carry) {
	f = fmaxf(incl_max(f, lane), carry);
	carry = __shfl(f, 63, 64);
	return f;
}

// The sorted union of A [na] and B [nb] (both non-decreasing), one output slot q at a time.  merge_split: i = the number of A's
// elements among the first q outputs, found by a merge-path search; with j = q - i the slot takes A[i] (from_a) or B[j].
// On equal values A_FIRST_ON_TIES puts A's element first (a stable cat([A, B]).sort()), otherwise B's
// (try_merge_two_packs_sorted_aligned: the lower bound of b among a); equal elements of one list keep their order either way.
// Every index read is in range by construction of the search interval, whatever the values are: lo <= mid < hi gives mid < na and
// 1 <= q - mid <= nb, and A[i] / B[j] are read behind their bound checks.
template <bool A_FIRST_ON_TIES>
__device__ __forceinline__ int merge_split(int q, int na, int nb, const float *A, const float *B) {
	int lo = max(0, q - nb), hi = min(q, na);
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (A_FIRST_ON_TIES ? A[mid] <= B[q - mid - 1] : A[mid] < B[q - mid - 1]) lo = mid + 1; else hi = mid;
	}
	return lo;
}
// the slot's indices, for a caller that scatters by them ...
struct Slot { int i, j; bool from_a; };
template <bool A_FIRST_ON_TIES>
__device__ __forceinline__ Slot merge_slot(int q, int na, int nb, const float *A, const float *B) {
	const int i = merge_split<A_FIRST_ON_TIES>(q, na, nb, A, B), j = q - i;
	return {i, j, i < na && (j >= nb || (A_FIRST_ON_TIES ? A[i] <= B[j] : A[i] < B[j]))};
}
// ... and its value alone (nerf_upsample.hip: through the struct its stage kernel comes out 0.6 % slower on one path, through this
// form byte for byte as with the merge written out; profiles/wave_row.md)
template <bool A_FIRST_ON_TIES>
__device__ __forceinline__ float merge_value(int q, int na, int nb, const float *A, const float *B) {
	const int i = merge_split<A_FIRST_ON_TIES>(q, na, nb, A, B), j = q - i;
	const bool from_a = i < na && (j >= nb || (A_FIRST_ON_TIES ? A[i] <= B[j] : A[i] < B[j]));
	return from_a ? A[i] : B[j];
}

}  // namespace wave_row
}  // namespace nr3d
