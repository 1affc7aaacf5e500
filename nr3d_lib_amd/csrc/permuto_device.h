// nr3d_lib_amd/csrc/permuto_device.h -- permutohedral-lattice encoder (PermutoSDF's encoding) for gfx950: the kernels, templated on
// the input dimension D, the pseudo-level width PW (2 or 4: the vector width of every table read / scatter) and the table dtype.
// Reference: csrc/permuto/include/permuto/permuto_cuda.h (kernel_permutohedral :124-330, kernel_permutohedral_backward_lattice
// :333-545, kernel_permutohedral_backward_input :548-770, kernel_permutohedral_backward_backward_input :772-1030).
//
// Every kernel recomputes the point's simplex per level from x (the reference's measured choice: storing rank / rem0 costs more
// than recomputing them, permuto/tests/compare_save_intermediate.py).  The operations that decide the simplex -- elevation, the
// nearest remainder-0 point, the ranks and the `sum` correction -- are the reference's, in its order, in fp32 without contraction
// (the Makefile's -ffp-contract=off), so a point lands in the same simplex and hashes to the same table rows.
//
// Differences from the reference kernels (results agree to fp32 rounding):
//  * one thread per (point, ACTUAL level) walking the level's features in chunks of PW, not one thread per pseudo level: a
//    4-feature level of a [4, 2, ...] meta finds its simplex once, not twice;
//  * the reference's rank-indexed arrays (barycentric[D - rank[d]], dL_dbarycentric[...]) are written through selects over the
//    rank (sort_by_rank, pick, put): a dynamic index into a register array becomes scratch memory on gfx950;
//  * fp16 tables are read as half and used as float; y and dL/d(dL_dy) are summed in fp32 and rounded once, dL/dparam is
//    accumulated in fp32 (the reference sums y in half and scatters with __half2 atomics) -- DESIGN §7;
//  * dL/dx sums the levels of a point in registers (one thread per point) and writes every column once, zeros from max_pos_dims
//    up and for skipped points (the reference: one fp32 atomic per point, level and column into a zero-filled buffer);
//  * skipped levels / points are WRITTEN as zeros in y and dL/d(dL_dy) (the reference leaves a zero-filled buffer alone), so the
//    bindings may allocate them uninitialised.
#pragma once
#include "common.h"

namespace nr3d {
namespace permuto {

static constexpr int kBlock = 256;

// by-value kernel argument: what the kernels need of nr3d_permuto_meta_t (reference: PermutoEncMetaRef, permuto_cuda.h:49-86)
struct DevMeta {
	uint32_t level_offsets[NR3D_PERMUTO_MAX_LEVELS + 1];
	uint32_t level_sizes[NR3D_PERMUTO_MAX_LEVELS];
	uint32_t level_n_feats[NR3D_PERMUTO_MAX_LEVELS];
	uint32_t level_cols[NR3D_PERMUTO_MAX_LEVELS];
	uint32_t n_levels, n_encoded_dims, n_params;
};

// the arguments of every launch (one struct: the per-dimension instantiation files see one signature)
struct Args {
	DevMeta m;
	uint32_t n;
	int param_dtype;
	const float *x, *scales, *shifts;
	const void *params;
	const int64_t *bidx, *boffs;
	uint32_t bds;
	int32_t max_level;
	uint32_t max_pos_dims;
	const void *gy; int64_t gy_sn, gy_se;        // dL_dy (params dtype)
	const float *ggx;                            // dL_ddLdx [n, D]
	void *y; int64_t y_sn, y_se;                 // y, or dL_ddLdy (params dtype)
	float *dx;                                   // dL_dx [n, D]
	float *dp;                                   // dL_dparam f32, zero-init
	hipStream_t st;
};

enum Op { OP_FWD = 0, OP_BWD_DX = 1, OP_BWD_DPARAM = 2, OP_BWD_BWD = 3 };

template <typename P, int PW> struct alignas(sizeof(P) * PW) Vec { P v[PW]; };

// element offset of the point's table set, false for a skipped point (batch_inds < 0); permuto_cuda.h:168-182
__device__ __forceinline__ bool batch_base(uint32_t i, const int64_t *bidx, const int64_t *boffs, uint32_t bds, uint32_t n_params,
                                           int64_t &base) {
	int64_t b = 0;
	if (bidx) {
		b = bidx[i];
		if (b < 0) return false;
	} else if (bds) {
		b = i / bds;
	}
	base = boffs ? boffs[b] : b * (int64_t)n_params;
	return true;
}

// The point's simplex at one level: elevated coordinates, the remainder-0 vertex and the ranks (permuto_cuda.h:203-264, same
// operations in the same order)
template <int D> struct Simplex {
	float elev[D + 1];
	int32_t rem0[D + 1];
	int32_t rank[D + 1];

	__device__ __forceinline__ void compute(const float *pos, const float *sc, const float *sh) {
		float sm = 0.f;
#pragma unroll
		for (int dim = D; dim > 0; dim--) {
			const float shift = sh ? sh[dim - 1] : 0.f;
			const float cf = (pos[dim - 1] + shift) * sc[dim - 1];
			elev[dim] = sm - (float)dim * cf;
			sm += cf;
		}
		elev[0] = sm;
		int32_t sum = 0;
#pragma unroll
		for (int dim = 0; dim <= D; ++dim) {
			const float v = elev[dim] / (float)(D + 1);
			const int32_t down = (int32_t)floorf(v) * (int32_t)(D + 1);
			const int32_t up = down + (int32_t)(D + 1);
			rem0[dim] = ((float)up - elev[dim] < elev[dim] - (float)down) ? up : down;
			sum += rem0[dim];
			rank[dim] = 0;
		}
		sum /= (int32_t)(D + 1);
#pragma unroll
		for (int dim = 0; dim < D; ++dim) {
			const float di = elev[dim] - (float)rem0[dim];
#pragma unroll
			for (int o = dim + 1; o <= D; ++o) {
				if (di < elev[o] - (float)rem0[o]) rank[dim]++;
				else rank[o]++;
			}
		}
#pragma unroll
		for (int dim = 0; dim <= D; ++dim) {
			rank[dim] += sum;
			if (rank[dim] < 0) { rank[dim] += D + 1; rem0[dim] += D + 1; }
			else if (rank[dim] > D) { rank[dim] -= D + 1; rem0[dim] -= D + 1; }
		}
	}

	// table row of the remainder-k vertex (permuto_cuda.h:300-311: key over the first D coordinates, hash, % size)
	__device__ __forceinline__ uint32_t row(int k, uint32_t size) const {
		uint32_t h = 0;
#pragma unroll
		for (int dim = 0; dim < D; ++dim) {
			int32_t key = rem0[dim] + k;
			if (rank[dim] > D - k) key -= D + 1;
			h += (uint32_t)key;
			h *= 2531011u;
		}
		return h % size;
	}

	// out[r] = in[d] of the coordinate d whose rank is r (the rank is a permutation of 0..D)
	__device__ __forceinline__ void sort_by_rank(const float in[D + 1], float out[D + 1]) const {
#pragma unroll
		for (int r = 0; r <= D; ++r) {
			float v = 0.f;
#pragma unroll
			for (int d = 0; d <= D; ++d) v = rank[d] == r ? in[d] : v;
			out[r] = v;
		}
	}

	// barycentric weights of the D+1 vertices (permuto_cuda.h:283-292): b[D - rank[d]] += delta[d], b[D + 1 - rank[d]] -= delta[d],
	// b[0] += 1 + b[D + 1].  Each b[k] receives exactly one + and one - term, so the sum is order-free.
	__device__ __forceinline__ void weights(float w[D + 1]) const {
		float delta[D + 1], sd[D + 1];
#pragma unroll
		for (int d = 0; d <= D; ++d) delta[d] = (elev[d] - (float)rem0[d]) / (float)(D + 1);
		sort_by_rank(delta, sd);
		w[0] = sd[D] + (1.0f + (-sd[0]));
#pragma unroll
		for (int k = 1; k <= D; ++k) w[k] = sd[D - k] - sd[D + 1 - k];
	}
};

// arr[idx] for a run-time idx without a dynamic register index (folds to a plain read when idx is a compile-time constant)
template <int N> __device__ __forceinline__ float pick(const float arr[N], int idx) {
	float v = 0.f;
#pragma unroll
	for (int j = 0; j < N; ++j) v = j == idx ? arr[j] : v;
	return v;
}
template <int N> __device__ __forceinline__ void put(float arr[N], int idx, float v) {
#pragma unroll
	for (int j = 0; j < N; ++j) arr[j] = j == idx ? v : arr[j];
}

// the vertex loops are unrolled up to 16 input dimensions (D + 1 = 17 vertices); beyond, the loop stays and pick/put select
template <int D> struct Unroll { static constexpr int K = D <= 16 ? D + 1 : 1; };

// ---- forward (kernel_permutohedral, permuto_cuda.h:124-330): y[i, col_l + f] = sum_k w_k * table_l[row_k, f] -----------------
template <int D, int PW, typename P>
__global__ void __launch_bounds__(kBlock) k_permuto_fwd(const DevMeta m, uint32_t n, const float *__restrict__ x,
                                                        const P *__restrict__ params, const float *__restrict__ scales,
                                                        const float *__restrict__ shifts, const int64_t *__restrict__ bidx,
                                                        const int64_t *__restrict__ boffs, uint32_t bds, int32_t max_level,
                                                        P *__restrict__ y, int64_t y_sn, int64_t y_se) {
	constexpr int KU = Unroll<D>::K;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t l = blockIdx.y;
	const uint32_t nf = m.level_n_feats[l];
	P *yo = y + (int64_t)i * y_sn + (int64_t)m.level_cols[l] * y_se;
	int64_t base = 0;
	if ((int32_t)l > max_level || !batch_base(i, bidx, boffs, bds, m.n_params, base)) {
		for (uint32_t f = 0; f < nf; ++f) yo[f * y_se] = from_f32<P>(0.f);
		return;
	}
	Simplex<D> s;
	s.compute(x + (int64_t)i * D, scales + l * D, shifts ? shifts + l * D : nullptr);
	float w[D + 1];
	s.weights(w);
	const P *tab = params + base + m.level_offsets[l];
	const uint32_t size = m.level_sizes[l];
	for (uint32_t c = 0; c < nf; c += PW) {
		float acc[PW];
#pragma unroll
		for (int f = 0; f < PW; ++f) acc[f] = 0.f;
#pragma unroll KU
		for (int k = 0; k <= D; ++k) {
			const Vec<P, PW> v = *(const Vec<P, PW> *)(tab + s.row(k, size) * nf + c);
			const float wk = pick<D + 1>(w, k);
#pragma unroll
			for (int f = 0; f < PW; ++f) acc[f] += wk * to_f32<P>(v.v[f]);
		}
#pragma unroll
		for (int f = 0; f < PW; ++f) yo[(c + f) * y_se] = from_f32<P>(acc[f]);
	}
}

// ---- dL/dparam (kernel_permutohedral_backward_lattice, permuto_cuda.h:333-545): table_l[row_k, f] += w_k * dL_dy[i, col_l + f] ----
template <int D, int PW, typename P>
__global__ void __launch_bounds__(kBlock) k_permuto_bwd_dparam(const DevMeta m, uint32_t n, const float *__restrict__ x,
                                                               const float *__restrict__ scales, const float *__restrict__ shifts,
                                                               const int64_t *__restrict__ bidx, const int64_t *__restrict__ boffs,
                                                               uint32_t bds, int32_t max_level, const P *__restrict__ gy,
                                                               int64_t gy_sn, int64_t gy_se, float *__restrict__ dp) {
	constexpr int KU = Unroll<D>::K;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t l = blockIdx.y;
	int64_t base = 0;
	if ((int32_t)l > max_level || !batch_base(i, bidx, boffs, bds, m.n_params, base)) return;
	const uint32_t nf = m.level_n_feats[l];
	Simplex<D> s;
	s.compute(x + (int64_t)i * D, scales + l * D, shifts ? shifts + l * D : nullptr);
	float w[D + 1];
	s.weights(w);
	float *tab = dp + base + m.level_offsets[l];
	const P *g = gy + (int64_t)i * gy_sn + (int64_t)m.level_cols[l] * gy_se;
	const uint32_t size = m.level_sizes[l];
	for (uint32_t c = 0; c < nf; c += PW) {
		float gf[PW];
#pragma unroll
		for (int f = 0; f < PW; ++f) gf[f] = to_f32<P>(g[(c + f) * gy_se]);
#pragma unroll KU
		for (int k = 0; k <= D; ++k) {
			float *t = tab + s.row(k, size) * nf + c;
			const float wk = pick<D + 1>(w, k);
#pragma unroll
			for (int f = 0; f < PW; ++f) atomic_add_f32(t + f, gf[f] * wk);
		}
	}
}

// ---- dL/dx (kernel_permutohedral_backward_input, permuto_cuda.h:548-770): dL/dy -> dL/dB -> dL/dE -> dL/dx, one thread per point,
// the levels summed in registers ------------------------------------------------------------------------------------------------
template <int D, int PW, typename P>
__global__ void __launch_bounds__(kBlock) k_permuto_bwd_dx(const DevMeta m, uint32_t n, const float *__restrict__ x,
                                                           const P *__restrict__ params, const float *__restrict__ scales,
                                                           const float *__restrict__ shifts, const int64_t *__restrict__ bidx,
                                                           const int64_t *__restrict__ boffs, uint32_t bds, int32_t max_level,
                                                           uint32_t max_pos_dims, const P *__restrict__ gy, int64_t gy_sn,
                                                           int64_t gy_se, float *__restrict__ dx) {
	constexpr int KU = Unroll<D>::K;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float acc[D];
#pragma unroll
	for (int d = 0; d < D; ++d) acc[d] = 0.f;
	int64_t base = 0;
	const bool live = batch_base(i, bidx, boffs, bds, m.n_params, base);
	const int32_t n_lv = live ? min((int32_t)m.n_levels, max_level + 1) : 0;
	for (int32_t l = 0; l < n_lv; ++l) {
		const uint32_t nf = m.level_n_feats[l];
		const float *sc = scales + l * D;
		Simplex<D> s;
		s.compute(x + (int64_t)i * D, sc, shifts ? shifts + l * D : nullptr);
		const P *tab = (const P *)params + base + m.level_offsets[l];
		const P *g = gy + (int64_t)i * gy_sn + (int64_t)m.level_cols[l] * gy_se;
		const uint32_t size = m.level_sizes[l];
		// dL/dB_k = sum_f table[row_k, f] * dL_dy[f], stored by rank: Bs[r] = dL/dB_{D - r}
		float Bs[D + 1];
#pragma unroll
		for (int r = 0; r <= D; ++r) Bs[r] = 0.f;
#pragma unroll KU
		for (int k = 0; k <= D; ++k) {
			const uint32_t r = s.row(k, size) * nf;
			float b = 0.f;
			for (uint32_t c = 0; c < nf; c += PW) {
				const Vec<P, PW> v = *(const Vec<P, PW> *)(tab + r + c);
#pragma unroll
				for (int f = 0; f < PW; ++f) b += to_f32<P>(v.v[f]) * to_f32<P>(g[(c + f) * gy_se]);
			}
			put<D + 1>(Bs, D - k, b);
		}
		// dL/dE[d] = dL/dB[D - rank[d]] / (D+1) - dL/dB[D + 1 - rank[d]] / (D+1), with dL/dB[D + 1] = dL/dB[0] (permuto_cuda.h:741-749)
		float dE[D + 1];
#pragma unroll
		for (int d = 0; d <= D; ++d) {
			float a = 0.f, bm = 0.f;
#pragma unroll
			for (int r = 0; r <= D; ++r) {
				a = s.rank[d] == r ? Bs[r] : a;
				bm = s.rank[d] == r ? Bs[r == 0 ? D : r - 1] : bm;
			}
			dE[d] = a / (float)(D + 1) - bm / (float)(D + 1);
		}
		// dL/dx[dim] = s[dim] * (sum_{o <= dim} dL/dE[o] - (dim + 1) dL/dE[dim + 1])  (permuto_cuda.h:751-762)
		float pre = 0.f;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			pre += dE[d];
			const float scd = sc[d];
			acc[d] += pre * scd - dE[d + 1] * scd * (float)(d + 1);
		}
	}
#pragma unroll
	for (int d = 0; d < D; ++d) dx[(int64_t)i * D + d] = d < (int)max_pos_dims ? acc[d] : 0.f;
}

// ---- double backward (kernel_permutohedral_backward_backward_input, permuto_cuda.h:772-1030): from dL/d(dL_dx) to dL/d(dL_dy) and
// dL/dparam.  dL/dE from dL_ddLdx (all D columns, as the reference), dL/dB from dL/dE, then per vertex
// dL_ddLdy[f] += dB_k * table[row_k, f] and table_grad[row_k, f] += dB_k * dL_dy[f] ------------------------------------------------
template <int D, int PW, typename P>
__global__ void __launch_bounds__(kBlock) k_permuto_bwd_bwd(const DevMeta m, uint32_t n, const float *__restrict__ x,
                                                            const P *__restrict__ params, const float *__restrict__ scales,
                                                            const float *__restrict__ shifts, const int64_t *__restrict__ bidx,
                                                            const int64_t *__restrict__ boffs, uint32_t bds, int32_t max_level,
                                                            const float *__restrict__ ggx, const P *__restrict__ gy, int64_t gy_sn,
                                                            int64_t gy_se, P *__restrict__ ggy, int64_t ggy_sn, int64_t ggy_se,
                                                            float *__restrict__ dp) {
	constexpr int KU = Unroll<D>::K;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t l = blockIdx.y;
	const uint32_t nf = m.level_n_feats[l];
	P *go = ggy ? ggy + (int64_t)i * ggy_sn + (int64_t)m.level_cols[l] * ggy_se : nullptr;
	int64_t base = 0;
	if ((int32_t)l > max_level || !batch_base(i, bidx, boffs, bds, m.n_params, base)) {
		if (go)
			for (uint32_t f = 0; f < nf; ++f) go[f * ggy_se] = from_f32<P>(0.f);
		return;
	}
	const float *sc = scales + l * D;
	Simplex<D> s;
	s.compute(x + (int64_t)i * D, sc, shifts ? shifts + l * D : nullptr);
	// dL/dE[o] = sum_{dim >= o} g[dim] s[dim] - o g[o-1] s[o-1]  (permuto_cuda.h:940-950)
	float gs[D], dE[D + 1];
#pragma unroll
	for (int d = 0; d < D; ++d) gs[d] = ggx[(int64_t)i * D + d] * sc[d];
	float suf = 0.f;
	dE[D] = 0.f;
#pragma unroll
	for (int o = D - 1; o >= 0; --o) {
		suf += gs[o];
		dE[o] = suf;
	}
#pragma unroll
	for (int d = 0; d < D; ++d) dE[d + 1] -= gs[d] * (float)(d + 1);
	// dL/dB[k] = q[D - k] - q[D + 1 - k], dL/dB[0] = q[D] - q[0], q[r] = dL/dE[d of rank r] / (D+1)  (permuto_cuda.h:952-960)
	float e1[D + 1], q[D + 1], dB[D + 1];
#pragma unroll
	for (int d = 0; d <= D; ++d) e1[d] = dE[d] / (float)(D + 1);
	s.sort_by_rank(e1, q);
	dB[0] = q[D] + (-q[0]);
#pragma unroll
	for (int k = 1; k <= D; ++k) dB[k] = q[D - k] - q[D + 1 - k];

	const P *tab = params + base + m.level_offsets[l];
	float *dtab = dp ? dp + base + m.level_offsets[l] : nullptr;
	const P *g = gy + (int64_t)i * gy_sn + (int64_t)m.level_cols[l] * gy_se;
	const uint32_t size = m.level_sizes[l];
	for (uint32_t c = 0; c < nf; c += PW) {
		float acc[PW], gf[PW];
#pragma unroll
		for (int f = 0; f < PW; ++f) { acc[f] = 0.f; gf[f] = dtab ? to_f32<P>(g[(c + f) * gy_se]) : 0.f; }
#pragma unroll KU
		for (int k = 0; k <= D; ++k) {
			const uint32_t r = s.row(k, size) * nf + c;
			const float bk = pick<D + 1>(dB, k);
			if (go) {
				const Vec<P, PW> v = *(const Vec<P, PW> *)(tab + r);
#pragma unroll
				for (int f = 0; f < PW; ++f) acc[f] += bk * to_f32<P>(v.v[f]);
			}
			if (dtab) {
#pragma unroll
				for (int f = 0; f < PW; ++f) atomic_add_f32(dtab + r + f, gf[f] * bk);
			}
		}
		if (go) {
#pragma unroll
			for (int f = 0; f < PW; ++f) go[(c + f) * ggy_se] = from_f32<P>(acc[f]);
		}
	}
}

template <int D, int PW, typename P> int launch(int op, const Args &a) {
	const dim3 grid_lv(div_up(a.n, kBlock), a.m.n_levels), grid_pt(div_up(a.n, kBlock));
	const P *params = (const P *)a.params;
	const P *gy = (const P *)a.gy;
	switch (op) {
	case OP_FWD:
		k_permuto_fwd<D, PW, P><<<grid_lv, kBlock, 0, a.st>>>(a.m, a.n, a.x, params, a.scales, a.shifts, a.bidx, a.boffs, a.bds,
		                                                       a.max_level, (P *)a.y, a.y_sn, a.y_se);
		break;
	case OP_BWD_DX:
		k_permuto_bwd_dx<D, PW, P><<<grid_pt, kBlock, 0, a.st>>>(a.m, a.n, a.x, params, a.scales, a.shifts, a.bidx, a.boffs, a.bds,
		                                                          a.max_level, a.max_pos_dims, gy, a.gy_sn, a.gy_se, a.dx);
		break;
	case OP_BWD_DPARAM:
		k_permuto_bwd_dparam<D, PW, P><<<grid_lv, kBlock, 0, a.st>>>(a.m, a.n, a.x, a.scales, a.shifts, a.bidx, a.boffs, a.bds,
		                                                              a.max_level, gy, a.gy_sn, a.gy_se, a.dp);
		break;
	case OP_BWD_BWD:
		k_permuto_bwd_bwd<D, PW, P><<<grid_lv, kBlock, 0, a.st>>>(a.m, a.n, a.x, params, a.scales, a.shifts, a.bidx, a.boffs, a.bds,
		                                                           a.max_level, a.ggx, gy, a.gy_sn, a.gy_se, (P *)a.y, a.y_sn, a.y_se,
		                                                           a.dp);
		break;
	default:
		return fail("permuto: unknown op %d", op);
	}
	NR3D_LAUNCH_CHECK();
	return 0;
}

template <int D> int launch_dim(int op, const Args &a, uint32_t pw) {
	const bool half = a.param_dtype == NR3D_F16;
	if (pw == 4) return half ? launch<D, 4, __half>(op, a) : launch<D, 4, float>(op, a);
	return half ? launch<D, 2, __half>(op, a) : launch<D, 2, float>(op, a);
}

// one per instantiation file (permuto_d{a..g}.hip): 1 if that file holds dimension D (and launched), else 0; < 0 on a launch error
int run_group_a(int D, int op, const Args &a, uint32_t pw, int *rc);
int run_group_b(int D, int op, const Args &a, uint32_t pw, int *rc);
int run_group_c(int D, int op, const Args &a, uint32_t pw, int *rc);
int run_group_d(int D, int op, const Args &a, uint32_t pw, int *rc);
int run_group_e(int D, int op, const Args &a, uint32_t pw, int *rc);
int run_group_f(int D, int op, const Args &a, uint32_t pw, int *rc);
int run_group_g(int D, int op, const Args &a, uint32_t pw, int *rc);

}  // namespace permuto
}  // namespace nr3d

// instantiation-file helper: `PERMUTO_GROUP(a, X(2) X(3) ...)`
#define NR3D_PERMUTO_CASE(Dv) case Dv: *rc = launch_dim<Dv>(op, a, pw); return 1;
#define NR3D_PERMUTO_GROUP(name, CASES)                                                            \
	namespace nr3d { namespace permuto {                                                            \
	int run_group_##name(int D, int op, const Args &a, uint32_t pw, int *rc) {                      \
		switch (D) { CASES default: return 0; }                                                     \
	}                                                                                               \
	} }
