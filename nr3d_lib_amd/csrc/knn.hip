// nr3d_lib_amd/csrc/knn.hip -- brute-force k nearest neighbours between two batched point clouds and its backward (nr3d_knn_points,
// nr3d_knn_points_backward): the HIP twin of the reference's externals/pytorch3d_knn, behind nr3d_lib_amd/bindings/_pytorch3d_knn.py and
// nr3d_lib_amd/maths.  The contract (distance arithmetic, the (dist, j) order, padding, what non-finite coordinates may do) is in
// include/nr3d_hip.h; tests/knn_ref.py restates it in numpy.  A different design from the reference's kernels: no spatial index, no
// split of p2 over workgroups.
//
//   k_knn<D, KB, NORM, R>   the fast kernel: compile-time D in 1..8, K <= KB in {1, 4, 8, 16, 32}.  A lane owns R query points in
//       registers (R consecutive strips of the workgroup's rows, so that the loads of a strip coalesce); the p2 cloud of the workgroup's
//       batch element streams through LDS in tiles of kTile points, each point padded to 1, 2, 4 or 8 floats so that one ds_read_b32 /
//       b64 / b128 (two b128 for D > 4) fetches it.  Every lane of a wave reads the SAME address: a broadcast, no bank conflicts.
//       The running top-K of a query is a sorted list in statically indexed registers (every loop over it is fully unrolled; a
//       runtime-indexed array would go to scratch).  A candidate enters only on dist < worst, strictly, and then goes in front of the
//       strictly larger entries only (insert(): every slot decides for itself from two compares, which gives what a chain of
//       conditional swaps gives without its serial dependence): j only grows, so the list is in (dist, j) order and at the K-th
//       place the lower index wins.  K == 1 is one compare and two selects, no branch.
//   k_knn_any               every other (D, K): one lane per query, p2 from global memory, the candidate list in the row's own output
//       slots.  The same contract; correct and unoptimised.
//   k_knn_bwd               one lane per (n, i): grad_p1 is the lane's own sum in k order (one store, no atomics: deterministic),
//       grad_p2 takes -t through float32 atomic adds (zero-initialised by the caller).
//
// Compiled without contraction (Makefile): the one fused operation of the distance is the fmaf written out below.
#include "common.h"

namespace nr3d {
namespace knn {

constexpr int kMaxD = 8;                 // the fast kernel's dimensions
constexpr int kMaxKB = 32;               // its largest K bucket
#ifndef NR3D_KNN_TILE
#define NR3D_KNN_TILE 1024
#endif
#ifndef NR3D_KNN_WG
#define NR3D_KNN_WG 256
#endif
constexpr int kTile = NR3D_KNN_TILE;     // p2 points per LDS tile (16 KiB at D = 3; of 256 .. 2048, measured)
constexpr int kBlock = NR3D_KNN_WG;      // the largest workgroup (the host launches 64 .. kBlock lanes)
constexpr uint64_t kWantGroups = 512;    // two workgroups per CU: below it the host trades R, then the workgroup size, for more groups

// floats per LDS row
template <int D> struct Row { static constexpr int S = D == 1 ? 1 : D == 2 ? 2 : D <= 4 ? 4 : 8; };
// query points per lane of the wide variant, by bucket (the list takes 2 R KB registers)
#ifdef NR3D_KNN_R
template <int KB> struct Wide { static constexpr int R = KB >= 32 ? 1 : (NR3D_KNN_R); };
#else
template <int KB> struct Wide { static constexpr int R = KB == 1 ? 4 : KB <= 16 ? 2 : 1; };     // of 1, 2, 4, measured
#endif

__device__ __forceinline__ uint32_t clamp_len(const int64_t *lengths, uint32_t n, uint32_t P) {
	if (!lengths) return P;
	const int64_t v = lengths[n];
	return v < 0 ? 0u : (v > (int64_t)P ? P : (uint32_t)v);
}

// include/nr3d_hip.h: d_0 * d_0 then fmaf(d_c, d_c, dist) | |d_0| then dist + |d_c|
template <int D, int NORM>
__device__ __forceinline__ float dist_of(const float (&a)[D], const float *q) {
	const float d0 = a[0] - q[0];
	float dist = NORM == 2 ? d0 * d0 : fabsf(d0);
#pragma unroll
	for (int c = 1; c < D; ++c) {
		const float dc = a[c] - q[c];
		dist = NORM == 2 ? fmaf(dc, dc, dist) : dist + fabsf(dc);
	}
	return dist;
}

template <int S>
__device__ __forceinline__ void read_row(const float *tile, uint32_t jj, float (&q)[S]) {
	if constexpr (S == 1) {
		q[0] = tile[jj];
	} else if constexpr (S == 2) {
		const float2 v = *reinterpret_cast<const float2 *>(tile + 2 * jj);
		q[0] = v.x; q[1] = v.y;
	} else {
#pragma unroll
		for (int h = 0; h < S / 4; ++h) {
			const float4 v = *reinterpret_cast<const float4 *>(tile + S * jj + 4 * h);
			q[4 * h] = v.x; q[4 * h + 1] = v.y; q[4 * h + 2] = v.z; q[4 * h + 3] = v.w;
		}
	}
}

// selects on VALUES: `c ? x[i] : x[j]` on two array elements is an lvalue conditional, which the compiler turns into one load through a
// selected index -- a runtime index into the list, resolved by a select chain over all of it (measured in the disassembly: 1220
// instructions per insertion at KB = 16)
__device__ __forceinline__ float sel(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ int sel(bool c, int a, int b) { return c ? a : b; }

// the candidate (d, j) into the sorted list: slot s takes its upper neighbour when the candidate belongs above that neighbour, the
// candidate when it belongs exactly here, and keeps its entry otherwise.  Every compare is strict, so the candidate lands BEHIND the
// entries of equal distance (which have lower j), and a NaN distance changes nothing.  The slots do not depend on each other: KB
// independent steps of one compare and four selects, not a chain of KB swaps.
template <int KB>
__device__ __forceinline__ void insert(float (&bd)[KB], int (&bi)[KB], float d, int j) {
	if constexpr (KB == 1) {
		const bool lt = d < bd[0];
		bd[0] = sel(lt, d, bd[0]);
		bi[0] = sel(lt, j, bi[0]);
	} else {
		if (d < bd[KB - 1]) {
#pragma unroll
			for (int s = KB - 1; s > 0; --s) {
				const float up = bd[s - 1], cur = bd[s];
				const int iup = bi[s - 1], icur = bi[s];
				const bool above = d < up, here = d < cur;
				bd[s] = sel(above, up, sel(here, d, cur));
				bi[s] = sel(above, iup, sel(here, j, icur));
			}
			const bool first = d < bd[0];
			bd[0] = sel(first, d, bd[0]);
			bi[0] = sel(first, j, bi[0]);
		}
	}
}

template <int D, int KB, int NORM, int R>
__global__ __launch_bounds__(kBlock) void k_knn(const float *__restrict__ p1, const float *__restrict__ p2,
                                                const int64_t *__restrict__ lengths1, const int64_t *__restrict__ lengths2, uint32_t P1,
                                                uint32_t P2, uint32_t K, uint32_t groups_per_cloud, float *__restrict__ dists,
                                                int64_t *__restrict__ idx) {
	constexpr int S = Row<D>::S;
	constexpr int U = KB == 1 ? 8 : KB <= 4 ? 4 : 2;
	__shared__ __attribute__((aligned(16))) float tile[kTile * S];
	const uint32_t n = blockIdx.x / groups_per_cloud, g = blockIdx.x % groups_per_cloud;
	const uint32_t wg = blockDim.x, tid = threadIdx.x;
	const uint32_t len1 = clamp_len(lengths1, n, P1);
	const uint32_t first = g * wg * (uint32_t)R;                  // < P1: groups_per_cloud = ceil(P1 / (wg R))
	const uint32_t len2 = first < len1 ? clamp_len(lengths2, n, P2) : 0u;      // a group of padding rows only: nothing to search

	float a[R][D];
	float bd[R][KB];
	int bi[R][KB];
#pragma unroll
	for (int r = 0; r < R; ++r) {
		const uint32_t i = first + (uint32_t)r * wg + tid;
#pragma unroll
		for (int c = 0; c < D; ++c) a[r][c] = i < P1 ? p1[((size_t)n * P1 + i) * D + c] : 0.f;
#pragma unroll
		for (int k = 0; k < KB; ++k) { bd[r][k] = __builtin_inff(); bi[r][k] = 0; }
	}

	for (uint32_t t0 = 0; t0 < len2; t0 += kTile) {
		const uint32_t cnt = min((uint32_t)kTile, len2 - t0);
		const float *__restrict__ src = p2 + ((size_t)n * P2 + t0) * D;
		__syncthreads();                                          // the previous tile has been consumed
		for (uint32_t e = tid; e < cnt * D; e += wg) tile[(e / D) * S + (e % D)] = src[e];
		__syncthreads();
#pragma unroll U
		for (uint32_t jj = 0; jj < cnt; ++jj) {
			float q[S];
			read_row<S>(tile, jj, q);
#pragma unroll
			for (int r = 0; r < R; ++r) insert<KB>(bd[r], bi[r], dist_of<D, NORM>(a[r], q), (int)(t0 + jj));
		}
	}

	const uint32_t kk = min(K, len2);
#pragma unroll
	for (int r = 0; r < R; ++r) {
		const uint32_t i = first + (uint32_t)r * wg + tid;
		if (i >= P1) continue;
		const bool live = i < len1;
		float *__restrict__ od = dists + ((size_t)n * P1 + i) * K;
		int64_t *__restrict__ oi = idx + ((size_t)n * P1 + i) * K;
#pragma unroll
		for (int k = 0; k < KB; ++k) {
			if ((uint32_t)k < K) {
				const bool have = live && (uint32_t)k < kk;
				od[k] = have ? bd[r][k] : 0.f;
				oi[k] = have ? (int64_t)bi[r][k] : (int64_t)0;
			}
		}
	}
}

// every other (D, K): one lane per query, p2 from global memory, the list in the row's own output slots; correct and unoptimised.  What
// it does do: the worst kept distance lives in a register, so a pair that does not enter reads nothing of the list; candidates are
// taken four at a time, so that their loads are in flight together; for D <= 8 (DC = D; DC = 0: any D) the query sits in registers.
constexpr int kAnyBlock = 64;
template <int DC>
__global__ __launch_bounds__(kAnyBlock) void k_knn_any(const float *__restrict__ p1, const float *__restrict__ p2,
                                                       const int64_t *__restrict__ lengths1, const int64_t *__restrict__ lengths2,
                                                       uint64_t rows, uint32_t P1, uint32_t P2, uint32_t D_, uint32_t K, int norm,
                                                       float *dists, int64_t *idx) {
	const uint64_t row = (uint64_t)blockIdx.x * kAnyBlock + threadIdx.x;
	if (row >= rows) return;
	const uint32_t D = DC ? (uint32_t)DC : D_;
	const uint32_t n = (uint32_t)(row / P1), i = (uint32_t)(row % P1);
	float *rd = dists + row * K;
	int64_t *ri = idx + row * K;
	uint32_t have = 0;
	if (i < clamp_len(lengths1, n, P1)) {
		const uint32_t len2 = clamp_len(lengths2, n, P2);
		const float *__restrict__ a = p1 + row * D;
		float areg[DC ? DC : 1];
		if constexpr (DC != 0) {
#pragma unroll
			for (int c = 0; c < DC; ++c) areg[c] = a[c];
		}
		float worst = 0.f;                                        // rd[K - 1] once the list is full
		for (uint32_t j0 = 0; j0 < len2; j0 += 4) {
			float dist[4];
#pragma unroll
			for (uint32_t u = 0; u < 4; ++u) {
				const float *__restrict__ q = p2 + ((size_t)n * P2 + min(j0 + u, len2 - 1)) * D;
				float a0;
				if constexpr (DC != 0) a0 = areg[0]; else a0 = a[0];
				const float d0 = a0 - q[0];
				float acc = norm == 2 ? d0 * d0 : fabsf(d0);
				if constexpr (DC != 0) {
#pragma unroll
					for (int c = 1; c < DC; ++c) {
						const float dc = areg[c] - q[c];
						acc = norm == 2 ? fmaf(dc, dc, acc) : acc + fabsf(dc);
					}
				} else {
					for (uint32_t c = 1; c < D; ++c) {
						const float dc = a[c] - q[c];
						acc = norm == 2 ? fmaf(dc, dc, acc) : acc + fabsf(dc);
					}
				}
				dist[u] = acc;
			}
#pragma unroll
			for (uint32_t u = 0; u < 4; ++u) {
				const uint32_t j = j0 + u;
				const float d = dist[u];
				if (j >= len2) continue;
				uint32_t s;
				if (have < K) s = have++;
				else if (d < worst) s = K - 1;
				else continue;
				// one step of an insertion sort, stopping at the first entry that is not larger (walking the whole list so that the loads
				// do not wait for the compares was measured and is slower, 47 against 35 ms at 2^14 x 2^14, K = 40: the walk is bound by
				// its memory transactions, 64 cache lines per wave and slot, not by their latency)
				for (; s > 0 && d < rd[s - 1]; --s) { rd[s] = rd[s - 1]; ri[s] = ri[s - 1]; }
				rd[s] = d; ri[s] = (int64_t)j;
				if (have == K) worst = rd[K - 1];
			}
		}
	}
	for (uint32_t k = have; k < K; ++k) { rd[k] = 0.f; ri[k] = 0; }
}

__global__ __launch_bounds__(256) void k_knn_bwd(const float *__restrict__ p1, const float *__restrict__ p2,
                                                 const int64_t *__restrict__ lengths1, const int64_t *__restrict__ lengths2,
                                                 const int64_t *__restrict__ idx, const float *__restrict__ grad_dists, uint64_t rows,
                                                 uint32_t P1, uint32_t P2, uint32_t D, uint32_t K, int norm, float *__restrict__ grad_p1,
                                                 float *__restrict__ grad_p2) {
	const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (row >= rows) return;
	const uint32_t n = (uint32_t)(row / P1), i = (uint32_t)(row % P1);
	const uint32_t kk = i < clamp_len(lengths1, n, P1) ? min(K, clamp_len(lengths2, n, P2)) : 0u;
	const float *__restrict__ a = p1 + row * D;
	const int64_t *__restrict__ ri = idx + row * K;
	const float *__restrict__ rg = grad_dists + row * K;
	for (uint32_t c = 0; c < D; ++c) {
		float sum = 0.f;
		for (uint32_t k = 0; k < kk; ++k) {
			const int64_t j = ri[k];
			if (j < 0 || j >= (int64_t)P2) continue;              // not an index of knn_points: nothing is read or written through it
			const size_t at = ((size_t)n * P2 + (size_t)j) * D + c;
			const float b = p2[at], gk = rg[k];
			const float t = norm == 2 ? (2.f * gk) * (a[c] - b) : (a[c] > b ? gk : -gk);
			sum = sum + t;
			atomic_add_f32(grad_p2 + at, -t);
		}
		grad_p1[row * D + c] = sum;
	}
}

struct Args {
	const float *p1, *p2;
	const int64_t *lengths1, *lengths2;
	uint64_t N;
	uint32_t P1, P2, K;
	float *dists;
	int64_t *idx;
	hipStream_t st;
};

template <int D, int KB, int NORM, int R>
static int launch_r(const Args &a, uint32_t wg) {
	const uint32_t per_cloud = div_up(a.P1, (uint64_t)wg * R);
	const uint64_t groups = a.N * per_cloud;
	NR3D_CHECK(groups < (1ull << 31), "knn_points: N = %llu clouds of %u points are %llu workgroups, fewer than 2^31 per call (split the batch)",
	           (unsigned long long)a.N, a.P1, (unsigned long long)groups);
	hipLaunchKernelGGL((k_knn<D, KB, NORM, R>), dim3((uint32_t)groups), dim3(wg), 0, a.st, a.p1, a.p2, a.lengths1, a.lengths2, a.P1, a.P2, a.K,
	                   per_cloud, a.dists, a.idx);
	NR3D_LAUNCH_CHECK();
	return 0;
}

// the launch plan of the fast kernel, pure host arithmetic: what launch_kb launches and what nr3d_knn_launch_plan reports
struct Plan { uint32_t R, wg; };

// the K bucket of the fast kernel (K in 1 .. kMaxKB)
static uint32_t bucket_of(uint32_t K) { return K == 1 ? 1u : K <= 4 ? 4u : K <= 8 ? 8u : K <= 16 ? 16u : 32u; }

static uint32_t wide_r(uint32_t KB) {
	switch (KB) {
	case 1: return Wide<1>::R;
	case 4: return Wide<4>::R;
	case 8: return Wide<8>::R;
	case 16: return Wide<16>::R;
	default: return Wide<32>::R;
	}
}

// the wide variant (Wide<KB>::R queries per lane, kBlock lanes) when that still gives every CU two workgroups; else one query per lane, and
// then smaller workgroups, down to one wave
static Plan plan_of(uint64_t N, uint64_t P1, uint32_t KB) {
	const uint32_t RW = wide_r(KB);
	if (RW > 1 && N * div_up(P1, (uint64_t)kBlock * RW) >= kWantGroups) return Plan{RW, (uint32_t)kBlock};
	uint32_t wg = kBlock;
	while (wg > 64 && N * div_up(P1, wg) < kWantGroups) wg >>= 1;
	return Plan{1u, wg};
}

template <int D, int KB, int NORM>
static int launch_kb(const Args &a) {
	constexpr int RW = Wide<KB>::R;
	const Plan p = plan_of(a.N, a.P1, KB);
	if constexpr (RW > 1) {
		if (p.R == (uint32_t)RW) return launch_r<D, KB, NORM, RW>(a, p.wg);
	}
	return launch_r<D, KB, NORM, 1>(a, p.wg);
}

template <int D, int NORM>
static int launch_d(const Args &a) {
	switch (bucket_of(a.K)) {
	case 1: return launch_kb<D, 1, NORM>(a);
	case 4: return launch_kb<D, 4, NORM>(a);
	case 8: return launch_kb<D, 8, NORM>(a);
	case 16: return launch_kb<D, 16, NORM>(a);
	default: return launch_kb<D, 32, NORM>(a);
	}
}

template <int NORM>
static int launch_norm(const Args &a, uint32_t D) {
	switch (D) {
	case 1: return launch_d<1, NORM>(a);
	case 2: return launch_d<2, NORM>(a);
	case 3: return launch_d<3, NORM>(a);
	case 4: return launch_d<4, NORM>(a);
	case 5: return launch_d<5, NORM>(a);
	case 6: return launch_d<6, NORM>(a);
	case 7: return launch_d<7, NORM>(a);
	default: return launch_d<8, NORM>(a);
	}
}

static int check_args(const char *fn, uint64_t N, uint64_t P1, uint64_t P2, uint32_t D, uint32_t K, int norm) {
	NR3D_CHECK(P1 < (1ull << 31) && P2 < (1ull << 31), "%s: P1 = %llu, P2 = %llu points per cloud, fewer than 2^31 each", fn,
	           (unsigned long long)P1, (unsigned long long)P2);
	NR3D_CHECK(N < (1ull << 31), "%s: N = %llu clouds, fewer than 2^31 per call", fn, (unsigned long long)N);
	NR3D_CHECK(K >= 1, "%s: K = 0, at least one neighbour", fn);
	NR3D_CHECK(D >= 1, "%s: D = 0, at least one coordinate", fn);
	NR3D_CHECK(norm == 1 || norm == 2, "%s: norm = %d, 1 (L1) or 2 (squared L2)", fn, norm);
	return 0;
}

}  // namespace knn
}  // namespace nr3d

using namespace nr3d;

extern "C" int nr3d_knn_fast_path(uint32_t D, uint32_t K) {
	return D >= 1 && D <= (uint32_t)knn::kMaxD && K >= 1 && K <= (uint32_t)knn::kMaxKB ? 1 : 0;
}

extern "C" int nr3d_knn_tile_points(uint32_t D) { return D >= 1 && D <= (uint32_t)knn::kMaxD ? knn::kTile : 0; }

extern "C" int nr3d_knn_launch_plan(uint64_t N, uint64_t P1, uint32_t D, uint32_t K) {
	if (!nr3d_knn_fast_path(D, K)) return 0;
	const knn::Plan p = knn::plan_of(N, P1, knn::bucket_of(K));
	return (int)(p.R | p.wg << 8);
}

extern "C" int nr3d_knn_points(const float *p1, const float *p2, const int64_t *lengths1, const int64_t *lengths2, uint64_t N, uint64_t P1,
                               uint64_t P2, uint32_t D, uint32_t K, int norm, float *dists, int64_t *idx, void *stream) {
	NR3D_TRY(knn::check_args("knn_points", N, P1, P2, D, K, norm));
	if (N == 0 || P1 == 0 || P2 == 0) return 0;
	NR3D_CHECK(p1 && p2 && dists && idx, "knn_points: NULL p1 / p2 / dists / idx");
	hipStream_t st = (hipStream_t)stream;
	if (nr3d_knn_fast_path(D, K)) {
		const knn::Args a{p1, p2, lengths1, lengths2, N, (uint32_t)P1, (uint32_t)P2, K, dists, idx, st};
		return norm == 2 ? knn::launch_norm<2>(a, D) : knn::launch_norm<1>(a, D);
	}
	const uint64_t rows = N * P1, groups = (rows + knn::kAnyBlock - 1) / knn::kAnyBlock;
	NR3D_CHECK(groups < (1ull << 31), "knn_points: %llu query points, fewer than 2^37 per call on the generic kernel (split the batch)",
	           (unsigned long long)rows);
#define NR3D_KNN_ANY(DC) hipLaunchKernelGGL(knn::k_knn_any<DC>, dim3((uint32_t)groups), dim3(knn::kAnyBlock), 0, st, p1, p2, lengths1, lengths2, \
	                                            rows, (uint32_t)P1, (uint32_t)P2, D, K, norm, dists, idx)
	switch (D) {
	case 1: NR3D_KNN_ANY(1); break;
	case 2: NR3D_KNN_ANY(2); break;
	case 3: NR3D_KNN_ANY(3); break;
	case 4: NR3D_KNN_ANY(4); break;
	case 5: NR3D_KNN_ANY(5); break;
	case 6: NR3D_KNN_ANY(6); break;
	case 7: NR3D_KNN_ANY(7); break;
	case 8: NR3D_KNN_ANY(8); break;
	default: NR3D_KNN_ANY(0); break;
	}
#undef NR3D_KNN_ANY
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_knn_points_backward(const float *p1, const float *p2, const int64_t *lengths1, const int64_t *lengths2, const int64_t *idx,
                                        const float *grad_dists, uint64_t N, uint64_t P1, uint64_t P2, uint32_t D, uint32_t K, int norm,
                                        float *grad_p1, float *grad_p2, void *stream) {
	NR3D_TRY(knn::check_args("knn_points_backward", N, P1, P2, D, K, norm));
	if (N == 0 || P1 == 0 || P2 == 0) return 0;
	NR3D_CHECK(p1 && p2 && idx && grad_dists && grad_p1 && grad_p2, "knn_points_backward: NULL p1 / p2 / idx / grad_dists / grad_p1 / grad_p2");
	const uint64_t rows = N * P1, groups = (rows + 255) / 256;
	NR3D_CHECK(groups < (1ull << 31), "knn_points_backward: %llu query points, fewer than 2^39 per call (split the batch)", (unsigned long long)rows);
	hipLaunchKernelGGL(knn::k_knn_bwd, dim3((uint32_t)groups), dim3(256), 0, (hipStream_t)stream, p1, p2, lengths1, lengths2, idx, grad_dists, rows,
	                   (uint32_t)P1, (uint32_t)P2, D, K, norm, grad_p1, grad_p2);
	NR3D_LAUNCH_CHECK();
	return 0;
}
