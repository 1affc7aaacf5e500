// nr3d_lib_amd/csrc/mlp_bwd.h -- what the fp32 backward kernels of the fused decoder share: mlp.hip (k_mlp_bwd, k_mlp_bwd2) and
// mlp_softplus2.hip (k_mlp_bwd2_sp, a translation unit of its own: the ReLU / linear kernels keep their code object, and the two compile
// side by side).  Device side: the per-wave [feature][sample] LDS tiles, the sample contraction, the ReLU mask bits, the reduction of
// the waves' parameter gradients.  Host side: the fp32 sizes of the packed buffer and the launch plan of a backward kernel.
#pragma once
#include "common.h"
#include "mlp_device.h"      // register map, dense layers, loads and stores
#include "mlp_plan.h"        // the host-side plan shared with mlp_half.hip

namespace nr3d {
namespace mlp {

// ---------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------

constexpr int kTS = 36;                        // row stride (floats) of the per-wave [feature][sample] LDS tiles:
                                               // 16-byte aligned rows, and 8 consecutive rows cover all 32 banks

// register map -> [feature][sample] tile (rows of kTS floats)
template <int MAXT>
__device__ __forceinline__ void write_tile(float *__restrict__ T, int nt, const f16v (&r)[MAXT], int lane) {
	const int s = lane & 31, h = lane >> 5;
#pragma unroll
	for (int t = 0; t < MAXT; ++t) {
		if (t >= nt) continue;
#pragma unroll
		for (int j = 0; j < 16; ++j) T[(32 * t + 8 * (j >> 2) + 4 * h + (j & 3)) * kTS + s] = r[t][j];
	}
}

// 16 samples (half-wave h: samples 16h .. 16h+15) of row `row` -> MFMA operand values of the sample contraction
__device__ __forceinline__ void read_row16(const float *__restrict__ T, int row, int h, float (&v)[16]) {
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const f4v t4 = *reinterpret_cast<const f4v *>(T + row * kTS + 16 * h + 4 * q);
#pragma unroll
		for (int b = 0; b < 4; ++b) v[4 * q + b] = t4[b];
	}
}

// eight consecutive samples of a [feature][sample] tile row as the three bf16 pieces of an MFMA operand (mlp_device.h split3)
__device__ __forceinline__ void split3_row8(const float *__restrict__ src, bf8 (&p)[3], float &sum) {
	const f4v lo = *reinterpret_cast<const f4v *>(src), hi = *reinterpret_cast<const f4v *>(src + 4);
	const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
	for (int e = 0; e < 8; e += 2) {
		split3_pair<false>(v[e], v[e + 1], e, p);
		sum += v[e] + v[e + 1];
	}
}

// sum one layer's gradient accumulators over the waves of the workgroup (through LDS) and add them to global memory
template <int NO, int NI>
__device__ __forceinline__ void reduce_layer(const f16v (&dW)[NO][NI], const float (&db)[NO], float *__restrict__ R, float *gW, float *gb,
                                             uint32_t out_dim, uint32_t in_dim, int lane, int wave, int nw) {
	float *Rb = R + NO * NI * 1024;
	for (int w = 0; w < nw; ++w) {
		if (wave == w) {
#pragma unroll
			for (int ot = 0; ot < NO; ++ot) {
				Rb[ot * 64 + lane] = (w == 0 ? 0.0f : Rb[ot * 64 + lane]) + db[ot];
#pragma unroll
				for (int it = 0; it < NI; ++it)
#pragma unroll
					for (int j = 0; j < 16; ++j) {
						const int e = (((ot * NI + it) * 16 + j) << 6) + lane;
						R[e] = (w == 0 ? 0.0f : R[e]) + dW[ot][it][j];
					}
			}
		}
		__syncthreads();
	}
	for (uint32_t e = threadIdx.x; e < (uint32_t)(NO * NI * 1024); e += blockDim.x) {
		const uint32_t ln = e & 63u, j = (e >> 6) & 15u, it = (e >> 10) % NI, ot = (e >> 10) / NI;
		const uint32_t k = 32u * it + (ln & 31u), o = 32u * ot + 8u * (j >> 2) + 4u * (ln >> 5) + (j & 3u);
		if (o < out_dim && k < in_dim) atomic_add_f32(gW + (size_t)o * in_dim + k, R[e]);
	}
	if (gb)
		for (uint32_t e = threadIdx.x; e < (uint32_t)(NO * 32); e += blockDim.x) {
			const uint32_t o = e;                                       // 32 ot + row
			if (o < out_dim) atomic_add_f32(gb + o, Rb[(e >> 5) * 64 + (e & 31u)] + Rb[(e >> 5) * 64 + 32 + (e & 31u)]);
		}
	__syncthreads();
}

template <int NT>
__device__ __forceinline__ void zero_tiles(f16v (&r)[NT]) {
#pragma unroll
	for (int t = 0; t < NT; ++t)
#pragma unroll
		for (int j = 0; j < 16; ++j) r[t][j] = 0.0f;
}

// the ReLU mask of a register-map tile set as bits (bit 16 t + j = element j of tile t is positive), and its application: one
// v_bfe_i32 (0 or all ones) and one v_and_b32 per element -- +0.0 where the unit is off, as the "? g : 0.0f" of bwd_layer
template <int NT>
__device__ __forceinline__ uint32_t relu_bits(const f16v (&r)[NT]) {
	static_assert(NT <= 2, "16 bits per tile, 32 per lane");
	uint32_t m = 0;
#pragma unroll
	for (int t = 0; t < NT; ++t)
#pragma unroll
		for (int j = 0; j < 16; ++j) m |= (r[t][j] > 0.0f ? 1u : 0u) << (16 * t + j);
	return m;
}
template <int NT>
__device__ __forceinline__ void mask_bits(f16v (&r)[NT], uint32_t m) {
#pragma unroll
	for (int t = 0; t < NT; ++t)
#pragma unroll
		for (int j = 0; j < 16; ++j) {
			const int keep = (int)(m << (31 - (16 * t + j))) >> 31;
			const float v = r[t][j];                   // (a copy: __builtin_bit_cast of a vector element reads element 0)
			r[t][j] = __builtin_bit_cast(float, __builtin_bit_cast(int, v) & keep);
		}
}

// bwd_layer's contraction without the bias sums: dW += dPre^T . T over the wave's 32 samples, TG holding dPre (NO tiles), TB the
// tangent of the layer's input (NI tiles), both as [feature][sample]
template <int NO, int NI, bool X3>
__device__ __forceinline__ void contract_tiles(const float *__restrict__ TG, const float *__restrict__ TB, f16v (&dW)[NO][NI],
                                               int r, int h) {
	if constexpr (X3) {
		constexpr int PW[6] = {2, 0, 1, 1, 0, 0}, PX[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
		for (int st = 0; st < 2; ++st) {
			bf8 ap[NO][3], bp[NI][3];
			float dummy = 0.0f;
#pragma unroll
			for (int ot = 0; ot < NO; ++ot) split3_row8(TG + (32 * ot + r) * kTS + 16 * st + 8 * h, ap[ot], dummy);
#pragma unroll
			for (int it = 0; it < NI; ++it) split3_row8(TB + (32 * it + r) * kTS + 16 * st + 8 * h, bp[it], dummy);
#pragma unroll
			for (int t = 0; t < 6; ++t)
#pragma unroll
				for (int ot = 0; ot < NO; ++ot)
#pragma unroll
					for (int it = 0; it < NI; ++it)
						dW[ot][it] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[ot][PW[t]], bp[it][PX[t]], dW[ot][it], 0, 0, 0);
		}
	} else {
		float bv[NI][16];
#pragma unroll
		for (int it = 0; it < NI; ++it) read_row16(TB, 32 * it + r, h, bv[it]);
#pragma unroll
		for (int ot = 0; ot < NO; ++ot) {
			float av[16];
			read_row16(TG, 32 * ot + r, h, av);
#pragma unroll
			for (int it = 0; it < NI; ++it)
#pragma unroll
				for (int t = 0; t < 16; ++t) dW[ot][it] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[it][t], dW[ot][it], 0, 0, 0);
		}
	}
}

// x / v: row-major (any alignment: load_rows) or feature-major (load_cols_fast); no prefetch variants -- the x and v of the SDF step
// come in different layouts (x feature-major from the LoTD forward or 35-float rows, v whatever the eikonal term's backward made)
template <int NT>
__device__ __forceinline__ void load_xv(const float *__restrict__ p, int64_t s, uint32_t fm, uint32_t vec, uint32_t dim, uint64_t row,
                                        uint64_t n, int lane, f16v (&r)[NT]) {
	if (fm) load_cols_fast<NT>(p, s, dim, row < n ? row : n - 1, lane, r);     // rows past n: dL/dy (hence every r_l) is zero there
	else load_rows<NT>(p, s, dim, row, row < n, vec != 0, lane, r);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static uint64_t packed_floats(const Shape &s) {
	return (uint64_t)layer_floats(s.in_t, s.w_t) + (uint64_t)(s.n_layers - 2) * layer_floats(s.w_t, s.w_t) + layer_floats(s.w_t, s.out_t);
}

// ---------------------------------------------------------------------------------------------
// fp32 forward on the bf16 MFMA (round 5, "x3"): every fp32 value is split into three bf16 pieces, v = v1 + v2 + v3 with
// v1 = bf16(v), v2 = bf16(v - v1), v3 = bf16(v - v1 - v2) (24 significant bits; the subtractions are exact), and a product is the
// six piece products whose magnitude is above 2^-25 of it: w1 x1 + (w1 x2 + w2 x1) + (w2 x2 + w1 x3 + w3 x1), each exact in the
// multiplier and accumulated in fp32 by v_mfma_f32_32x32x16_bf16 -- the result is fp32-grade (dropped terms <= 2^-26 of a product,
// below the rounding of an fp32 multiply), at 6 MFMAs of 8 passes per K = 16 where the f32 MFMA needs 8 of 16 passes: 2.7x the
// matrix rate of v_mfma_f32_32x32x2_f32, which bounds csrc/mlp.hip's forward (0.55-0.63 of its 157 TFLOP/s).
// The weights' pieces are made once at pack time, in the operand order of csrc/mlp_half.hip (A of step s, lane (out i, h),
// element e = W[i][32 it + 8 (2 s + (e >> 2)) + 4 h + (e & 3)]); the activations' pieces per layer from the register map (a step's
// B operand = eight consecutive accumulator registers).  Region of the packed buffer: behind the f32 forward layers.
// ---------------------------------------------------------------------------------------------
static uint64_t x3_floats(const Shape &s) {
	const uint64_t n = (uint64_t)layer_x3_floats(s.in_t, s.w_t) + (uint64_t)(s.n_layers - 2) * layer_x3_floats(s.w_t, s.w_t) + layer_x3_floats(s.w_t, s.out_t);
	return n * 4 <= (uint64_t)kMaxLds ? n : 0;          // a network whose pieces do not fit LDS keeps the f32 MFMA
}
static bool x3_enabled() { return opt::on(NR3D_OPT_MLP_X3); }

// the f32 backward's LDS copy of the forward layers (mlp_device.h kGS / kHS)
static uint64_t padded_floats(const Shape &s) {
	return (uint64_t)layer_floats_pad(s.in_t, s.w_t) + (uint64_t)(s.n_layers - 2) * layer_floats_pad(s.w_t, s.w_t) + layer_floats_pad(s.w_t, s.out_t);
}

static uint64_t padded_x3_floats(const Shape &s) {
	return (uint64_t)layer_x3_floats_pad(s.in_t, s.w_t) + (uint64_t)(s.n_layers - 2) * layer_x3_floats_pad(s.w_t, s.w_t) + layer_x3_floats_pad(s.w_t, s.out_t);
}

// per-wave [feature][sample] tiles: X, H_1 .. H_NH, G_out
static uint32_t bwd_tile_floats(const Shape &s) { return (32u * (s.in_t > s.out_t ? s.in_t : s.out_t) + (s.n_layers - 1) * 32u * s.w_t) * (uint32_t)kTS; }

// weights the backward keeps in LDS: one padded copy of the forward layers, f32 or (x3) their bf16 planes
static uint64_t bwd_weight_floats(const Shape &s, bool x3) { return x3 ? padded_x3_floats(s) : padded_floats(s); }

// the launch of k_mlp_bwd / k_mlp_bwd2 on a network backward_ok() admits: as many waves as fit next to the weights (nw == 0: none, or
// x3 asked for a network without x3 planes)
static BwdPlan bwd_plan_of(const Shape &s, bool x3, uint64_t n = 0) {
	if (x3 && x3_floats(s) == 0) return {0, 0, 0};
	return bwd_plan(bwd_weight_floats(s, x3) * 4, (uint64_t)bwd_tile_floats(s) * 4, s.w_t,
	                bwd_max_waves_f32(s.in_t, s.w_t, s.out_t, s.n_layers - 1), 1, 0, n);
}

// Does the x3 option put the backward on the bf16 MFMA?  The kernel is not bound by its MFMAs -- counters of 32 -> 64 -> 64 -> 16
// (profiles/r06_mlp_counters.txt): VALU active 45 % of a wave's cycles (the piece splitting), MFMA pipe 31 %, one wave per SIMD
// overlaps little of it -- so a wave lost to the bigger planes costs more than the cheaper products bring: x3 where its planes
// (1.5 x the f32 bytes + padding) leave as many waves as the f32 copy.  Same-box A/B at 2^22 samples, fwd+bwd ms, x3 / f32:
// 32->64->64->16 1.90 / 2.33, 32->64->16 1.00 / 1.18, 32->32->16 0.60 / 0.63, 18->32->3 0.57 / 0.75; 64->64->64->64 x3 has three waves
// against four: 5.49 / 3.96 -> f32 (so do 64->64->64 and 32->64->64->64).  Until the transposing read (dense_x3_t) the small shapes
// kept a second, transposed set of planes in LDS (every weight read 16 bytes): equal within 2 % now, and gone.
static bool backward_x3(const Shape &s) {
	if (!bwd_has_x3(s.in_t, s.w_t, s.out_t, s.n_layers - 1)) return false;          // no x3 kernel is built for these (mlp_plan.h)
	const uint32_t w0 = bwd_plan_of(s, false).nw, w3 = bwd_plan_of(s, true).nw;
	return w3 != 0 && w3 >= w0;
}

}  // namespace mlp
}  // namespace nr3d
