// nr3d_lib_amd/csrc/mlp.hip -- fused fully-connected decoder (gfx950), C-ABI entry points
// nr3d_mlp_packed_floats / nr3d_mlp_pack / nr3d_mlp_forward / nr3d_mlp_backward / nr3d_mlp_backward_backward.
//
// The step right after the encoder: nr3d_lib/models/blocks/mlp.py:27-127 (`MLP` / `FCBlock`: D hidden
// DenseLayers of width W + an output layer, nr3d_lib/models/layers.py:228-300) -- in the reference a chain of
// cuBLAS GEMMs + elementwise kernels, or tiny-cuda-nn's fused fp16 MLP behind tcnn_adapter.py.  Here: fp32 in, fp32
// accumulate on the f32 MFMA (v_mfma_f32_32x32x2_f32: bitwise an fmaf chain, so parity with an fp32 reference is
// round-off only), the whole network in ONE kernel: activations never leave registers.
//
// Layout trick: everything is computed TRANSPOSED, H^T[feature, sample] = W . X^T, per wave on a tile of 32 samples.
// The MFMA's C/D map puts sample = lane & 31 in every lane and features 8a + 4(lane >> 5) + b (a, b < 4) in its 16
// accumulator registers; its B operand wants sample = lane & 31 and one k per half-wave.  Feeding register j of the
// previous layer's accumulator as B of step j means half-wave h contributes feature 8(j>>2) + 4h + (j&3) -- a fixed
// permutation of k, absorbed into the order the weights are packed in.  So the output registers of one layer ARE the
// input operands of the next: no LDS round trip, no shuffles.  The input X and the output Y use the same map, which
// makes every lane read / write 16-byte pieces of its sample's row.
// Weights (packed once per step by k_mlp_pack into MFMA operand order, zero padded to 32-wide tiles) sit in LDS.
//
// Backward recomputes the forward from X (keeping the activations in registers), walks the layers down with
// dH^T = W^T . dY^T on the same register map, and accumulates dW = dH^T . H_prev over the wave's samples: that
// product contracts over SAMPLES, which the register map has in the lane index, so both operands go through a
// per-wave LDS transposition tile ([feature][sample] -> one sample pair per MFMA step).
//
// Host side: what does not depend on the precision -- tile classes, eligibility, the backward's wave count / LDS bytes / grid, layout
// flags, the pack launches' layer table -- is csrc/mlp_plan.h, shared with csrc/mlp_half.hip; csrc/mlp_bwd.h adds the fp32 sizes and
// the device helpers of the backward kernels, which csrc/mlp_softplus2.hip (nr3d_mlp_softplus_backward_backward) uses too.
#include "common.h"
#include "mlp_device.h"      // register map, dense layers (f32 MFMA / bf16 MFMA x3), loads and stores
#include "mlp_plan.h"        // the host-side plan shared with mlp_half.hip: shape, dispatch, backward launch plan, layouts
#include "mlp_bwd.h"         // shared with mlp_softplus2.hip (the double backward of softplus hidden layers): LDS tiles, contraction, fp32 sizes and plan
#include <type_traits>

namespace nr3d {
namespace mlp {

// ---------------------------------------------------------------------------------------------
// packing: for layer l, packed[(((ot*NI + it)*4 + a)*64 + lane)*4 + b] = W[32 ot + (lane & 31)][32 it + 8a + 4(lane >> 5) + b]
// (no transposed layers are packed: the backward reads these transposed, mlp_device.h dense_t / dense_x3_t)
// ---------------------------------------------------------------------------------------------
struct PackArgs {
	const float *w[NR3D_MLP_MAX_LAYERS];
	const float *b[NR3D_MLP_MAX_LAYERS];
	uint32_t in_dim[NR3D_MLP_MAX_LAYERS], out_dim[NR3D_MLP_MAX_LAYERS];   // of W as stored: [out_dim, in_dim] row-major
	uint32_t ni[NR3D_MLP_MAX_LAYERS], no[NR3D_MLP_MAX_LAYERS];            // tiles of the packed layer's input / output
	uint32_t offset[NR3D_MLP_MAX_LAYERS + 1];                             // first float of every packed layer
	uint32_t n_layers;
};

__global__ __launch_bounds__(256) void k_mlp_pack(PackArgs a, float *__restrict__ packed) {
	const uint32_t l = blockIdx.y;
	const uint32_t nf = a.offset[l + 1] - a.offset[l];
	const uint32_t nw = a.no[l] * a.ni[l] * 1024u;
	for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < nf; e += gridDim.x * 256) {
		float v = 0.0f;
		if (e < nw) {
			const uint32_t b = e & 3u, lane = (e >> 2) & 63u, q = (e >> 8) & 3u, tile = e >> 10;
			const uint32_t it = tile % a.ni[l], ot = tile / a.ni[l];
			const uint32_t o = 32u * ot + (lane & 31u), f = 32u * it + 8u * q + 4u * (lane >> 5) + b;
			if (o < a.out_dim[l] && f < a.in_dim[l]) v = a.w[l][(size_t)o * a.in_dim[l] + f];
		} else if (a.b[l]) {
			const uint32_t o = e - nw;
			if (o < a.out_dim[l]) v = a.b[l][o];
		}
		packed[a.offset[l] + e] = v;
	}
}

// x3 planes of layer l: bf16 index e of plane p at ((((p * NO + ot) * NI + it) * 2 + s) * 64 + lane) * 8 + el; bias fp32 behind them
__global__ __launch_bounds__(256) void k_mlp_pack_x3(PackArgs a, float *__restrict__ packed) {
	const uint32_t l = blockIdx.y;
	const uint32_t nw = a.no[l] * a.ni[l] * 1024u;                        // weights of the (padded) layer
	__bf16 *wdst = reinterpret_cast<__bf16 *>(packed + a.offset[l]);
	float *bdst = packed + a.offset[l] + a.no[l] * a.ni[l] * 1536u;
	for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < nw + a.no[l] * 32u; e += gridDim.x * 256) {
		if (e < nw) {
			const uint32_t el = e & 7u, lane = (e >> 3) & 63u, st = (e >> 9) & 1u, tile = e >> 10;
			const uint32_t it = tile % a.ni[l], ot = tile / a.ni[l];
			const uint32_t o = 32u * ot + (lane & 31u), f = 32u * it + 8u * (2u * st + (el >> 2)) + 4u * (lane >> 5) + (el & 3u);
			float v = 0.0f;
			if (o < a.out_dim[l] && f < a.in_dim[l]) v = a.w[l][(size_t)o * a.in_dim[l] + f];
			const __bf16 p1 = (__bf16)v;
			const float r1 = v - (float)p1;
			const __bf16 p2 = (__bf16)r1;
			const __bf16 p3 = (__bf16)(r1 - (float)p2);
			wdst[e] = p1; wdst[nw + e] = p2; wdst[2u * nw + e] = p3;
		} else {
			const uint32_t o = e - nw;
			bdst[o] = (a.b[l] && o < a.out_dim[l]) ? a.b[l][o] : 0.0f;
		}
	}
}

// ---------------------------------------------------------------------------------------------
// one dense layer on the register map; wp -> LDS copy of the packed layer
// ---------------------------------------------------------------------------------------------
struct FwdArgs {
	uint64_t n;
	const float *x; int64_t xs;
	float *y; int64_t ys;
	const float *packed; uint32_t packed_floats;
	uint32_t n_layers, in_dim, out_dim;
	int hidden_act, out_act;
	uint32_t x_vec, y_vec;
	float beta;                                // of a softplus hidden activation (the SP instantiations)
};

// (X3, one input and one output tile, hidden layers up to 64 wide: two workgroups per CU = two waves per SIMD -- the piece splitting is VALU work, the products MFMA work, and
// only ANOTHER wave's instructions overlap them; at 260 registers the first version ran one wave per SIMD and the two added up)
// SP: the hidden activation is softplus (mlp_device.h hidden_layer); a.hidden_act is not read
// SG: the output activation is sigmoid (mlp_act.h), applied to the accumulators before store_rows; a.out_act is not read.  Instantiations
// of their own, like SP: as a third run-time case next to dense's ReLU test the sigmoid moved the registers of 187 of the 324 existing
// forward kernels (up to + 96 VGPRs on the 128-wide outputs) and of 80 of the 108 k_mlp_bwd (profiles/mlp_sigmoid_resources.txt)
template <int IN_T, int W_T, int OUT_T, int XF, bool X3 = false, bool SP = false, bool SG = false>
__global__ __launch_bounds__(kThreads, (X3 && IN_T == 1 && W_T <= 2 && OUT_T == 1) ? 2 : 1) void k_mlp_fwd(FwdArgs a) {
	extern __shared__ __attribute__((aligned(16))) float lds[];
	stage_weights(a.packed, a.packed_floats, lds);          // (X3: a.packed points at the x3 region, a.packed_floats is its size)
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t n_tiles = (a.n + 31) / 32, step = (uint64_t)gridDim.x * 4;
	const uint32_t off_hidden = X3 ? layer_x3_floats(IN_T, W_T) : layer_floats(IN_T, W_T), sz_hidden = X3 ? layer_x3_floats(W_T, W_T) : layer_floats(W_T, W_T);
	auto clamp_row = [&](uint64_t row) { return row < a.n ? row : a.n - 1; };
	f16v xnext[IN_T];
	if (XF) prefetch_x<XF, IN_T>(a.x, a.xs, a.in_dim, clamp_row(((uint64_t)blockIdx.x * 4 + wave) * 32 + (lane & 31)), lane, xnext);
	for (uint64_t tile = (uint64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += step) {
		const uint64_t row = tile * 32 + (lane & 31);
		const bool valid = row < a.n;
		f16v xin[IN_T], hcur[W_T], yo[OUT_T];
		if (XF) {
			// software pipeline: this tile's rows were requested one iteration ago, the next tile's go out now
#pragma unroll
			for (int t = 0; t < IN_T; ++t) xin[t] = xnext[t];
			prefetch_x<XF, IN_T>(a.x, a.xs, a.in_dim, clamp_row((tile + step) * 32 + (lane & 31)), lane, xnext);
		} else {
			load_rows<IN_T>(a.x, a.xs, a.in_dim, row, valid, a.x_vec != 0, lane, xin);
		}
		// wide networks (round 4): the LDS base goes through a register the compiler cannot see through, so that it does not hoist
		// every layer's weight fragments out of the tile loop (hundreds of loop-invariant registers -> 344 scratch instructions
		// in k_mlp_fwd<4, 4, 4, 2>, round-3 review)
		uint32_t opaque = 0;
		if constexpr (IN_T >= 4 || W_T >= 4 || OUT_T >= 4) asm volatile("s_mov_b32 %0, 0" : "=s"(opaque));
		const float *wl = lds + opaque;
		hidden_layer<IN_T, W_T, X3, false, SP>(wl, xin, hcur, a.hidden_act, a.beta, lane);
#pragma unroll 1
		for (uint32_t l = 1; l + 1 < a.n_layers; ++l) {
			f16v hn[W_T];
			hidden_layer<W_T, W_T, X3, false, SP>(wl + off_hidden + (l - 1) * sz_hidden, hcur, hn, a.hidden_act, a.beta, lane);
#pragma unroll
			for (int t = 0; t < W_T; ++t) hcur[t] = hn[t];
		}
		if constexpr (X3) dense_x3<W_T, OUT_T, true>(wl + off_hidden + (a.n_layers - 2) * sz_hidden, hcur, yo, SG ? (int)NR3D_MLP_ACT_NONE : a.out_act, lane);
		else dense<W_T, OUT_T, true>(wl + off_hidden + (a.n_layers - 2) * sz_hidden, hcur, yo, SG ? (int)NR3D_MLP_ACT_NONE : a.out_act, lane);
		if constexpr (SG) mlp_act::sigmoid_tiles<OUT_T>(yo);
		store_rows<OUT_T>(a.y, a.ys, a.out_dim, row, valid, a.y_vec != 0, lane, yo);
	}
}

// =============================================================================================
// backward: dL/dx (optional), dL/dW_l, dL/db_l from x and dL/dy, forward recomputed in registers
// =============================================================================================
struct BwdArgs {
	uint64_t n;
	const float *x; int64_t xs;
	const float *gy; int64_t gys;
	float *gx; int64_t gxs;                    // NULL: dL/dx not wanted
	uint32_t x_fm, gx_fm;                      // x is read / dL/dx is stored feature-major (xs / gxs = feature stride)
	const float *packed;                       // the forward layers: f32, or their x3 planes
	uint32_t total_floats;                     // of their padded LDS copy
	float beta;                                // of a softplus hidden activation (the SP instantiations); in the 4 bytes of padding in
	                                           // front of the pointers: the struct, hence the ReLU kernels' argument block, is unchanged
	float *dW[NR3D_MLP_MAX_LAYERS];            // accumulated into (atomics): zero them for plain gradients
	float *db[NR3D_MLP_MAX_LAYERS];            // may be NULL
	uint32_t dims[NR3D_MLP_MAX_LAYERS + 1];
	uint32_t n_layers;
	int hidden_act, out_act;
	uint32_t x_vec, gy_vec, gx_vec;
	uint32_t tile_floats;                      // per wave
};

// One layer of the backward sweep.  g = dL/d(pre-activation of this layer's output) on the register map (NO tiles);
// TG: LDS tile that receives g as [feature][sample]; TB: the layer's INPUT activations as [feature][sample] (NI tiles);
// wT: the padded LDS copy of THIS layer (read transposed).  Accumulates dW (NO x NI tiles) and the per-lane bias partial sums; when PREV, leaves
// dL/d(input of the layer) in gp, times the derivative of the input activations: MASK 1 = ReLU (H > 0), 2 = softplus with `beta`, which the
// same tile gives as -expm1(-beta H) (mlp_act.h), 0 = none.

template <int NO, int NI, bool PREV, int MASK, bool X3 = false>
__device__ __forceinline__ void bwd_layer(const f16v (&g)[NO], float *__restrict__ TG, const float *__restrict__ TB,
                                          const float *__restrict__ wT, f16v (&dW)[NO][NI], float (&db)[NO], f16v (&gp)[NI],
                                          int lane, float beta = 0.0f) {
	const int r = lane & 31, h = lane >> 5;
	write_tile<NO>(TG, NO, g, lane);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	if constexpr (X3) {
		// dW += dPre^T . H on the bf16 MFMA (round 6): the contraction runs over the tile's 32 samples = two K = 16 steps; lane (r, h) holds
		// samples 16 s + 8 h .. + 7 of row r of both operands, each split into three bf16 pieces, six piece products per step -- the
		// same fp32-grade sum as dense_x3 (smallest terms first), 12 MFMAs of 8 passes where the f32 MFMA takes 16 of 16 passes
		constexpr int PW[6] = {2, 0, 1, 1, 0, 0}, PX[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
		for (int st = 0; st < 2; ++st) {
			bf8 ap[NO][3], bp[NI][3];
			float dummy = 0.0f;
#pragma unroll
			for (int ot = 0; ot < NO; ++ot) split3_row8(TG + (32 * ot + r) * kTS + 16 * st + 8 * h, ap[ot], db[ot]);
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
			float sum = 0.0f;
#pragma unroll
			for (int t = 0; t < 16; ++t) sum += av[t];
			db[ot] += sum;
#pragma unroll
			for (int it = 0; it < NI; ++it)
#pragma unroll
				for (int t = 0; t < 16; ++t) dW[ot][it] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[it][t], dW[ot][it], 0, 0, 0);
		}
	}
	if (PREV) {
		if constexpr (X3) dense_x3_t<NO, NI>(wT, g, gp, lane);          // wT: the padded copy of the FORWARD layer's x3 planes
		else dense_t<NO, NI>(wT, g, gp, lane);                          //     ... of the forward layer
		if constexpr (MASK == 2) {
#pragma unroll
			for (int t = 0; t < NI; ++t)
#pragma unroll
				for (int j = 0; j < 16; ++j)
					gp[t][j] *= mlp_act::softplus_grad(TB[(32 * t + 8 * (j >> 2) + 4 * h + (j & 3)) * kTS + r], beta);
		} else if (MASK) {
#pragma unroll
			for (int t = 0; t < NI; ++t)
#pragma unroll
				for (int j = 0; j < 16; ++j)
					gp[t][j] = TB[(32 * t + 8 * (j >> 2) + 4 * h + (j & 3)) * kTS + r] > 0.0f ? gp[t][j] : 0.0f;
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// FAST: x and dL/dy rows are 16-byte aligned with widths that are multiples of 4 -> branch-free loads, the next tile's
// rows requested while this tile is processed (one wave per SIMD: nothing else hides the memory latency)
// FAST: 0 = any layout (row-major or, with a.x_fm, feature-major x), 1 = prefetched row-major x and dL/dy, 2 = prefetched
// feature-major x + row-major dL/dy
// Networks of 32-wide layers with <= 2 hidden layers leave room for EIGHT waves per workgroup, two per SIMD (round 4, as csrc/mlp_half.hip):
// the kernel is a chain of LDS round trips and dependent MFMAs per tile, a second wave per SIMD hides part of it.
template <int IN_T, int W_T, int OUT_T, int NH> struct BwdCfg { static constexpr int kMaxWaves = bwd_max_waves_f32(IN_T, W_T, OUT_T, NH); };
// X3 (round 6): the forward recomputation, the dH = W^T dPre chain and the sample contraction dW = dPre^T H all run on the bf16 MFMA with
// three-piece splits (dense_x3 / dense_x3_t / bwd_layer<..., true>); a.packed then points at the x3 planes of the forward layers.
// The ReLU masks come from the SAME forward arithmetic as nr3d_mlp_forward's x3 route.
// SP: softplus hidden layers (hidden_layer / bwd_layer<..., MASK = 2>): the H_l tiles kept for dW also give the derivative.
// (the ReLU / linear instantiations call dense / dense_x3 directly, not through hidden_layer: the extra inlining level alone moved the
// register allocation of four of them by 1 - 8 VGPRs and 7 spilled dwords)
// SG: sigmoid output (see k_mlp_fwd): the output pre-activations z are recomputed as for an output ReLU's mask, and dL/dy takes the factor
// sigmoid'(z) -- after the zeroing of the rows past n, which therefore stay zero; a.out_act is not read
template <int IN_T, int W_T, int OUT_T, int NH, int FAST, bool X3 = false, bool SP = false, bool SG = false>
__global__ __launch_bounds__((BwdCfg<IN_T, W_T, OUT_T, NH>::kMaxWaves * 64)) void k_mlp_bwd(BwdArgs a) {
	extern __shared__ __attribute__((aligned(16))) float lds[];
	// FAST: the next tile's rows are requested before a tile's LAST step, not at its top: their 32 - 64 registers then overlap one
	// layer's work instead of five (k_mlp_bwd<2,2,2,2>: 183 -> 139 / 220 -> 187 spilled dwords, 64 -> 64 -> 64 -> 64 4.38 -> 3.86 ms), and
	// one step still covers the latency (every measured shape equal or faster, 32 -> 32 -> 32 -> 16 0.66 -> 0.62 ms)
	{
		// ONE padded copy of the forward layers (f32, or their x3 planes) serves the forward recomputation (16-byte reads) and the
		// dH = W^T dPre chain (dense_t's 4-byte reads / dense_x3_t's transposing reads) -- no second, transposed copy: its LDS goes to
		// the waves' tiles.  On the f32 MFMA 64 -> 64 -> 64 -> 64 runs four waves per CU where two fitted; the x3 planes of
		// 32 -> 64 -> 64 -> 16 leave room for four waves where both orientations left two
		constexpr int GPP = X3 ? 6 : 4;
		constexpr uint32_t s0 = IN_T * W_T * GPP * 256 + W_T * 32, sh = W_T * W_T * GPP * 256 + W_T * 32;      // packed layers
		constexpr uint32_t GS = X3 ? kGS3 : kGS;
		constexpr uint32_t d0 = IN_T * W_T * GPP * GS + W_T * 32, dh = W_T * W_T * GPP * GS + W_T * 32;        // padded copies
		stage_layer_padded<IN_T, W_T, GPP>(a.packed, lds);
#pragma unroll
		for (int l = 1; l < NH; ++l) stage_layer_padded<W_T, W_T, GPP>(a.packed + s0 + (l - 1) * sh, lds + d0 + (l - 1) * dh);
		stage_layer_padded<W_T, OUT_T, GPP>(a.packed + s0 + (NH - 1) * sh, lds + d0 + (NH - 1) * dh);
		__syncthreads();
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
	const int r = lane & 31;
	float *tiles = lds + a.total_floats + (size_t)wave * a.tile_floats;
	// tile rows: X or G_out | H_1 .. H_NH.  G_out (dL/dy as [feature][sample]) lives from the output layer's step of the sweep to its
	// end, X from the first layer's step on -- the forward reads x from registers --, so they share their rows (round 6: the tile area
	// of 64 -> 64 -> 64 -> 64 drops from 36.9 to 27.6 KB per wave and TWO waves fit next to 98 KB of weights where one did;
	// 32 -> 64 -> 64 -> 16: four instead of three)
	constexpr int XG_T = IN_T > OUT_T ? IN_T : OUT_T;
	float *TX = tiles;
	float *TGO = tiles;
	float *TH1 = tiles + 32 * XG_T * kTS;                               // H_l at TH1 + (l - 1) * 32 * W_T * kTS
	// the padded layers: [0 | hidden ... | out]; the dH chain reads the same copies (wt + t0 + l th = layer l + 1)
	constexpr uint32_t f0 = X3 ? layer_x3_floats_pad(IN_T, W_T) : layer_floats_pad(IN_T, W_T);
	constexpr uint32_t fh = X3 ? layer_x3_floats_pad(W_T, W_T) : layer_floats_pad(W_T, W_T);
	constexpr uint32_t t0 = f0, th = fh;
	const float *wf = lds, *wt = lds;

	f16v dW0[W_T][IN_T], dWh[NH > 1 ? NH - 1 : 1][W_T][W_T], dWo[OUT_T][W_T];
	float db0[W_T], dbh[NH > 1 ? NH - 1 : 1][W_T], dbo[OUT_T];
#pragma unroll
	for (int ot = 0; ot < W_T; ++ot) { zero_tiles<IN_T>(dW0[ot]); db0[ot] = 0.0f; }
#pragma unroll
	for (int l = 0; l < (NH > 1 ? NH - 1 : 1); ++l)
#pragma unroll
		for (int ot = 0; ot < W_T; ++ot) { zero_tiles<W_T>(dWh[l][ot]); dbh[l][ot] = 0.0f; }
#pragma unroll
	for (int ot = 0; ot < OUT_T; ++ot) { zero_tiles<W_T>(dWo[ot]); dbo[ot] = 0.0f; }

	const uint64_t n_tiles = (a.n + 31) / 32, step = (uint64_t)gridDim.x * nw;
	auto clamp_row = [&](uint64_t row) { return row < a.n ? row : a.n - 1; };
	f16v xnext[IN_T], gnext[OUT_T];
	if (FAST) {
		const uint64_t r0 = clamp_row(((uint64_t)blockIdx.x * nw + wave) * 32 + r);
		prefetch_x<FAST, IN_T>(a.x, a.xs, a.dims[0], r0, lane, xnext);
		load_rows_fast<OUT_T>(a.gy, a.gys, a.dims[NH + 1], r0, lane, gnext);
	}
	for (uint64_t tile = (uint64_t)blockIdx.x * nw + wave; tile < n_tiles; tile += step) {
		const uint64_t row = tile * 32 + r;
		const bool valid = row < a.n;
		f16v xin[IN_T], g_out[OUT_T], hcur[W_T];
		if (FAST) {
#pragma unroll
			for (int t = 0; t < IN_T; ++t) xin[t] = xnext[t];
#pragma unroll
			for (int t = 0; t < OUT_T; ++t) g_out[t] = gnext[t];
		} else {
			if (a.x_fm) load_cols_fast<IN_T>(a.x, a.xs, a.dims[0], clamp_row(row), lane, xin);   // rows past n: dL/dy is zero there
			else load_rows<IN_T>(a.x, a.xs, a.dims[0], row, valid, a.x_vec != 0, lane, xin);
			load_rows<OUT_T>(a.gy, a.gys, a.dims[NH + 1], row, valid, a.gy_vec != 0, lane, g_out);
		}
		// ---- forward, activations kept as [feature][sample] tiles ----
		if constexpr (SP) hidden_layer<IN_T, W_T, X3, true, true>(wf, xin, hcur, a.hidden_act, a.beta, lane);
		else if constexpr (X3) dense_x3<IN_T, W_T, true, true>(wf, xin, hcur, a.hidden_act, lane);
		else dense<IN_T, W_T, true, true>(wf, xin, hcur, a.hidden_act, lane);
		write_tile<W_T>(TH1, W_T, hcur, lane);
#pragma unroll
		for (int l = 1; l < NH; ++l) {
			f16v hn[W_T];
			if constexpr (SP) hidden_layer<W_T, W_T, X3, true, true>(wf + f0 + (l - 1) * fh, hcur, hn, a.hidden_act, a.beta, lane);
			else if constexpr (X3) dense_x3<W_T, W_T, true, true>(wf + f0 + (l - 1) * fh, hcur, hn, a.hidden_act, lane);
			else dense<W_T, W_T, true, true>(wf + f0 + (l - 1) * fh, hcur, hn, a.hidden_act, lane);
#pragma unroll
			for (int t = 0; t < W_T; ++t) hcur[t] = hn[t];
			write_tile<W_T>(TH1 + l * 32 * W_T * kTS, W_T, hcur, lane);
		}
		if (FAST && !valid) zero_tiles<OUT_T>(g_out);                    // rows past n were clamped, not zeroed
		if constexpr (SG) {
			f16v yo[OUT_T];
			if constexpr (X3) dense_x3<W_T, OUT_T, true, true>(wf + f0 + (NH - 1) * fh, hcur, yo, NR3D_MLP_ACT_NONE, lane);
			else dense<W_T, OUT_T, true, true>(wf + f0 + (NH - 1) * fh, hcur, yo, NR3D_MLP_ACT_NONE, lane);
#pragma unroll
			for (int t = 0; t < OUT_T; ++t)
#pragma unroll
				for (int j = 0; j < 16; ++j) g_out[t][j] *= mlp_act::sigmoid_grad(yo[t][j]);
		} else if (a.out_act == NR3D_MLP_ACT_RELU) {
			f16v yo[OUT_T];
			if constexpr (X3) dense_x3<W_T, OUT_T, true, true>(wf + f0 + (NH - 1) * fh, hcur, yo, NR3D_MLP_ACT_NONE, lane);
			else dense<W_T, OUT_T, true, true>(wf + f0 + (NH - 1) * fh, hcur, yo, NR3D_MLP_ACT_NONE, lane);
#pragma unroll
			for (int t = 0; t < OUT_T; ++t)
#pragma unroll
				for (int j = 0; j < 16; ++j) g_out[t][j] = yo[t][j] > 0.0f ? g_out[t][j] : 0.0f;
		}
		// ---- backward sweep ----
		const bool relu = a.hidden_act == NR3D_MLP_ACT_RELU;
		f16v g[W_T];
		if constexpr (SP) bwd_layer<OUT_T, W_T, true, 2, X3>(g_out, TGO, TH1 + (NH - 1) * 32 * W_T * kTS, wt + t0 + (NH - 1) * th, dWo, dbo, g, lane, a.beta);
		else if (relu) bwd_layer<OUT_T, W_T, true, true, X3>(g_out, TGO, TH1 + (NH - 1) * 32 * W_T * kTS, wt + t0 + (NH - 1) * th, dWo, dbo, g, lane);
		else bwd_layer<OUT_T, W_T, true, false, X3>(g_out, TGO, TH1 + (NH - 1) * 32 * W_T * kTS, wt + t0 + (NH - 1) * th, dWo, dbo, g, lane);
		write_tile<IN_T>(TX, IN_T, xin, lane);                           // into G_out's rows: their reader, the step above, is done; x leaves the registers here
#pragma unroll
		for (int l = NH - 1; l >= 1; --l) {                              // hidden layer l: H_l -> H_{l+1}
			f16v gp[W_T];
			float *TG = TH1 + l * 32 * W_T * kTS;                       // H_{l+1} is dead once its mask has been applied
			const float *TB = TH1 + (l - 1) * 32 * W_T * kTS;
			if constexpr (SP) bwd_layer<W_T, W_T, true, 2, X3>(g, TG, TB, wt + t0 + (l - 1) * th, dWh[l - 1], dbh[l - 1], gp, lane, a.beta);
			else if (relu) bwd_layer<W_T, W_T, true, true, X3>(g, TG, TB, wt + t0 + (l - 1) * th, dWh[l - 1], dbh[l - 1], gp, lane);
			else bwd_layer<W_T, W_T, true, false, X3>(g, TG, TB, wt + t0 + (l - 1) * th, dWh[l - 1], dbh[l - 1], gp, lane);
#pragma unroll
			for (int t = 0; t < W_T; ++t) g[t] = gp[t];
		}
		if constexpr (FAST != 0) {                                       // the next tile's rows (see above)
			const uint64_t rn = clamp_row((tile + step) * 32 + r);
			prefetch_x<FAST, IN_T>(a.x, a.xs, a.dims[0], rn, lane, xnext);
			load_rows_fast<OUT_T>(a.gy, a.gys, a.dims[NH + 1], rn, lane, gnext);
		}
		f16v gx[IN_T];
		if (a.gx) {
			bwd_layer<W_T, IN_T, true, false, X3>(g, TH1, TX, wt, dW0, db0, gx, lane);
			if (a.gx_fm) store_cols<IN_T>(a.gx, a.gxs, a.dims[0], row, valid, lane, gx);
			else store_rows<IN_T>(a.gx, a.gxs, a.dims[0], row, valid, a.gx_vec != 0, lane, gx);
		} else {
			bwd_layer<W_T, IN_T, false, false, X3>(g, TH1, TX, wt, dW0, db0, gx, lane);
		}
	}

	// ---- reduce the waves' parameter gradients in LDS (the tile area is free now), one atomic per element ----
	__syncthreads();
	float *R = lds + a.total_floats;
	reduce_layer<W_T, IN_T>(dW0, db0, R, a.dW[0], a.db[0], a.dims[1], a.dims[0], lane, wave, nw);
#pragma unroll
	for (int l = 1; l < NH; ++l) reduce_layer<W_T, W_T>(dWh[l - 1], dbh[l - 1], R, a.dW[l], a.db[l], a.dims[l + 1], a.dims[l], lane, wave, nw);
	reduce_layer<OUT_T, W_T>(dWo, dbo, R, a.dW[NH], a.db[NH], a.dims[NH + 1], a.dims[NH], lane, wave, nw);
}

// =============================================================================================
// double backward (second order, the eikonal term of an SDF decoder): the network is piecewise linear, so with the ReLU masks m_l of
// the forward, r_l the first backward's dL/d(pre-activation of layer l) (r_L = m_L u, r_{l-1} = m_{l-1} W_l^T r_l) and the TANGENT of
// the incoming v = dL/d(dL/dx) through the same masks (t_{-1} = v, t_l = m_l W_l t_{l-1}, no bias):
//   dL/dW_l = sum over samples of r_l t_{l-1}^T,   dL/d(dL/dy) = t_L,   dL/db_l = 0,   dL/dx = 0 (sigma'' = 0 almost everywhere).
// k_mlp_bwd2 is k_mlp_bwd with the activation tiles H_l replaced by the tangent tiles t_l (same rows, same LDS, same waves) and the
// masks kept as one bit per register-map element instead of being read back from H_l > 0: the forward recomputation runs the same
// dense / dense_x3 as k_mlp_bwd (same X3 rule), so the masks are bit for bit the ones nr3d_mlp_backward used.  No db, no dL/dx.
// =============================================================================================
struct Bwd2Args {
	uint64_t n;
	const float *x; int64_t xs;
	const float *gy; int64_t gys;
	const float *v; int64_t vs;                // dL/d(dL/dx)
	float *ggy; int64_t ggys;                  // dL/d(dL/dy) [n, out] rows; NULL: not wanted
	uint32_t x_fm, v_fm;                       // x / v feature-major (xs / vs = feature stride)
	const float *packed;                       // the forward layers: f32, or their x3 planes
	uint32_t total_floats;                     // of their padded LDS copy
	float *dW[NR3D_MLP_MAX_LAYERS];            // accumulated into (atomics): zero them for plain gradients
	uint32_t dims[NR3D_MLP_MAX_LAYERS + 1];
	uint32_t n_layers;
	int hidden_act, out_act;
	uint32_t x_vec, gy_vec, v_vec, ggy_vec;
	uint32_t tile_floats;                      // per wave
};

// bwd_layer of the double backward: TB holds the tangent of the layer's input, the mask of dL/d(input) comes from bits
template <int NO, int NI, bool PREV, bool MASK, bool X3>
__device__ __forceinline__ void bwd2_layer(const f16v (&g)[NO], float *__restrict__ TG, const float *__restrict__ TB,
                                           const float *__restrict__ wT, f16v (&dW)[NO][NI], f16v (&gp)[NI], uint32_t mbits, int lane) {
	const int r = lane & 31, h = lane >> 5;
	write_tile<NO>(TG, NO, g, lane);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	contract_tiles<NO, NI, X3>(TG, TB, dW, r, h);
	if (PREV) {
		if constexpr (X3) dense_x3_t<NO, NI>(wT, g, gp, lane);
		else dense_t<NO, NI>(wT, g, gp, lane);
		if (MASK) mask_bits<NI>(gp, mbits);
	}
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

template <int IN_T, int W_T, int OUT_T, int NH, bool X3 = false>
__global__ __launch_bounds__((BwdCfg<IN_T, W_T, OUT_T, NH>::kMaxWaves * 64)) void k_mlp_bwd2(Bwd2Args a) {
	extern __shared__ __attribute__((aligned(16))) float lds[];
	{
		// the padded copy of the forward layers, as k_mlp_bwd
		constexpr int GPP = X3 ? 6 : 4;
		constexpr uint32_t s0 = IN_T * W_T * GPP * 256 + W_T * 32, sh = W_T * W_T * GPP * 256 + W_T * 32;
		constexpr uint32_t GS = X3 ? kGS3 : kGS;
		constexpr uint32_t d0 = IN_T * W_T * GPP * GS + W_T * 32, dh = W_T * W_T * GPP * GS + W_T * 32;
		stage_layer_padded<IN_T, W_T, GPP>(a.packed, lds);
#pragma unroll
		for (int l = 1; l < NH; ++l) stage_layer_padded<W_T, W_T, GPP>(a.packed + s0 + (l - 1) * sh, lds + d0 + (l - 1) * dh);
		stage_layer_padded<W_T, OUT_T, GPP>(a.packed + s0 + (NH - 1) * sh, lds + d0 + (NH - 1) * dh);
		__syncthreads();
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
	const int r = lane & 31;
	float *tiles = lds + a.total_floats + (size_t)wave * a.tile_floats;
	// tile rows as k_mlp_bwd: V (= t_{-1}) or G_out | T_1 .. T_NH (the tangents of the hidden layers' outputs, where k_mlp_bwd keeps H_l)
	constexpr int XG_T = IN_T > OUT_T ? IN_T : OUT_T;
	float *TV = tiles;
	float *TGO = tiles;
	float *TT1 = tiles + 32 * XG_T * kTS;
	constexpr uint32_t f0 = X3 ? layer_x3_floats_pad(IN_T, W_T) : layer_floats_pad(IN_T, W_T);
	constexpr uint32_t fh = X3 ? layer_x3_floats_pad(W_T, W_T) : layer_floats_pad(W_T, W_T);
	const float *wl = lds;

	f16v dW0[W_T][IN_T], dWh[NH > 1 ? NH - 1 : 1][W_T][W_T], dWo[OUT_T][W_T];
#pragma unroll
	for (int ot = 0; ot < W_T; ++ot) zero_tiles<IN_T>(dW0[ot]);
#pragma unroll
	for (int l = 0; l < (NH > 1 ? NH - 1 : 1); ++l)
#pragma unroll
		for (int ot = 0; ot < W_T; ++ot) zero_tiles<W_T>(dWh[l][ot]);
#pragma unroll
	for (int ot = 0; ot < OUT_T; ++ot) zero_tiles<W_T>(dWo[ot]);

	const bool relu = a.hidden_act == NR3D_MLP_ACT_RELU;
	const uint64_t n_tiles = (a.n + 31) / 32, step = (uint64_t)gridDim.x * nw;
	for (uint64_t tile = (uint64_t)blockIdx.x * nw + wave; tile < n_tiles; tile += step) {
		const uint64_t row = tile * 32 + r;
		const bool valid = row < a.n;
		f16v vin[IN_T], g_out[OUT_T], tcur[W_T];
		load_xv<IN_T>(a.v, a.vs, a.v_fm, a.v_vec, a.dims[0], row, a.n, lane, vin);
		// ---- forward: the masks only (one bit per element), the activations die layer by layer ----
		uint32_t mk[NH], mo = ~0u;
		{
			f16v xin[IN_T], hcur[W_T];
			load_xv<IN_T>(a.x, a.xs, a.x_fm, a.x_vec, a.dims[0], row, a.n, lane, xin);
			if constexpr (X3) dense_x3<IN_T, W_T, true, true>(wl, xin, hcur, a.hidden_act, lane);
			else dense<IN_T, W_T, true, true>(wl, xin, hcur, a.hidden_act, lane);
			mk[0] = relu ? relu_bits<W_T>(hcur) : 0u;
#pragma unroll
			for (int l = 1; l < NH; ++l) {
				f16v hn[W_T];
				if constexpr (X3) dense_x3<W_T, W_T, true, true>(wl + f0 + (l - 1) * fh, hcur, hn, a.hidden_act, lane);
				else dense<W_T, W_T, true, true>(wl + f0 + (l - 1) * fh, hcur, hn, a.hidden_act, lane);
				mk[l] = relu ? relu_bits<W_T>(hn) : 0u;
#pragma unroll
				for (int t = 0; t < W_T; ++t) hcur[t] = hn[t];
			}
			if (a.out_act == NR3D_MLP_ACT_RELU) {
				f16v yo[OUT_T];
				if constexpr (X3) dense_x3<W_T, OUT_T, true, true>(wl + f0 + (NH - 1) * fh, hcur, yo, NR3D_MLP_ACT_NONE, lane);
				else dense<W_T, OUT_T, true, true>(wl + f0 + (NH - 1) * fh, hcur, yo, NR3D_MLP_ACT_NONE, lane);
				mo = relu_bits<OUT_T>(yo);
			}
		}
		load_rows<OUT_T>(a.gy, a.gys, a.dims[NH + 1], row, valid, a.gy_vec != 0, lane, g_out);      // (under the tangent chain)
		// ---- the tangent of v through the same masks, T_l into the tiles ----
		if constexpr (X3) dense_x3<IN_T, W_T, false, true>(wl, vin, tcur, NR3D_MLP_ACT_NONE, lane);
		else dense<IN_T, W_T, false, true>(wl, vin, tcur, NR3D_MLP_ACT_NONE, lane);
		if (relu) mask_bits<W_T>(tcur, mk[0]);
		write_tile<W_T>(TT1, W_T, tcur, lane);
#pragma unroll
		for (int l = 1; l < NH; ++l) {
			f16v tn[W_T];
			if constexpr (X3) dense_x3<W_T, W_T, false, true>(wl + f0 + (l - 1) * fh, tcur, tn, NR3D_MLP_ACT_NONE, lane);
			else dense<W_T, W_T, false, true>(wl + f0 + (l - 1) * fh, tcur, tn, NR3D_MLP_ACT_NONE, lane);
			if (relu) mask_bits<W_T>(tn, mk[l]);
#pragma unroll
			for (int t = 0; t < W_T; ++t) tcur[t] = tn[t];
			write_tile<W_T>(TT1 + l * 32 * W_T * kTS, W_T, tcur, lane);
		}
		// ---- output layer: r_L = m_L u, dL/d(dL/dy) = t_L = m_L W_L t ----
		const float *wo = wl + f0 + (NH - 1) * fh;
		if (a.out_act == NR3D_MLP_ACT_RELU) mask_bits<OUT_T>(g_out, mo);
		if (a.ggy) {
			f16v to[OUT_T];
			if constexpr (X3) dense_x3<W_T, OUT_T, false, true>(wo, tcur, to, NR3D_MLP_ACT_NONE, lane);
			else dense<W_T, OUT_T, false, true>(wo, tcur, to, NR3D_MLP_ACT_NONE, lane);
			if (a.out_act == NR3D_MLP_ACT_RELU) mask_bits<OUT_T>(to, mo);
			store_rows<OUT_T>(a.ggy, a.ggys, a.dims[NH + 1], row, valid, a.ggy_vec != 0, lane, to);
		}
		// ---- adjoint sweep: dW_l += r_l t_{l-1}^T ----
		f16v g[W_T];
		if (relu) bwd2_layer<OUT_T, W_T, true, true, X3>(g_out, TGO, TT1 + (NH - 1) * 32 * W_T * kTS, wo, dWo, g, mk[NH - 1], lane);
		else bwd2_layer<OUT_T, W_T, true, false, X3>(g_out, TGO, TT1 + (NH - 1) * 32 * W_T * kTS, wo, dWo, g, 0u, lane);
		write_tile<IN_T>(TV, IN_T, vin, lane);                           // into G_out's rows (as x in k_mlp_bwd)
#pragma unroll
		for (int l = NH - 1; l >= 1; --l) {
			f16v gp[W_T];
			float *TG = TT1 + l * 32 * W_T * kTS;                       // T_{l+1} was last read by the step above
			const float *TB = TT1 + (l - 1) * 32 * W_T * kTS;
			if (relu) bwd2_layer<W_T, W_T, true, true, X3>(g, TG, TB, wl + f0 + (l - 1) * fh, dWh[l - 1], gp, mk[l - 1], lane);
			else bwd2_layer<W_T, W_T, true, false, X3>(g, TG, TB, wl + f0 + (l - 1) * fh, dWh[l - 1], gp, 0u, lane);
#pragma unroll
			for (int t = 0; t < W_T; ++t) g[t] = gp[t];
		}
		f16v unused[IN_T];
		bwd2_layer<W_T, IN_T, false, false, X3>(g, TT1, TV, wl, dW0, unused, 0u, lane);
	}

	// ---- reduce the waves' dW in LDS, one atomic per element (no db: the bias gradients of the double backward are zero) ----
	__syncthreads();
	float *R = lds + a.total_floats;
	float zb0[W_T], zbh[W_T], zbo[OUT_T];
#pragma unroll
	for (int t = 0; t < W_T; ++t) { zb0[t] = 0.0f; zbh[t] = 0.0f; }
#pragma unroll
	for (int t = 0; t < OUT_T; ++t) zbo[t] = 0.0f;
	reduce_layer<W_T, IN_T>(dW0, zb0, R, a.dW[0], nullptr, a.dims[1], a.dims[0], lane, wave, nw);
#pragma unroll
	for (int l = 1; l < NH; ++l) reduce_layer<W_T, W_T>(dWh[l - 1], zbh, R, a.dW[l], nullptr, a.dims[l + 1], a.dims[l], lane, wave, nw);
	reduce_layer<OUT_T, W_T>(dWo, zbo, R, a.dW[NH], nullptr, a.dims[NH + 1], a.dims[NH], lane, wave, nw);
}


}  // namespace mlp
}  // namespace nr3d

using namespace nr3d;
using namespace nr3d::mlp;

// the forward part of the packed buffer: [f32 layers | x3 planes of the same layers (0 floats when they do not fit LDS)]
static uint64_t forward_floats(const Shape &s) { return packed_floats(s) + x3_floats(s); }

extern "C" uint64_t nr3d_mlp_packed_floats(const nr3d_mlp_desc_t *desc) {
	Shape s;
	if (!shape_of(desc, s)) return 0;
	const uint64_t n = packed_floats(s);
	return n * 4 <= (uint64_t)kMaxLds ? forward_floats(s) : 0;      // 0: the fused kernels do not apply to this network
}

// behind the forward part: kBwdHeader floats (non-zero size = "the fused backward applies"; the backward reads the forward layers)
constexpr uint32_t kBwdHeader = 4;
extern "C" uint64_t nr3d_mlp_backward_packed_floats(const nr3d_mlp_desc_t *desc) {
	Shape s;
	if (!shape_of(desc, s) || nr3d_mlp_packed_floats(desc) == 0 || !backward_ok(s) || bwd_plan_of(s, false).nw == 0) return 0;
	return kBwdHeader;
}

extern "C" int nr3d_mlp_pack(const nr3d_mlp_desc_t *desc, const float *const *weights, const float *const *biases, float *packed,
                             int with_backward, void *stream) {
	Shape s;
	NR3D_CHECK(shape_of(desc, s) && nr3d_mlp_packed_floats(desc) != 0, "mlp_pack: network outside the fused kernels' range "
	           "(2..%d linear layers, every width 1..128, packed weights <= %d KB)", NR3D_MLP_MAX_LAYERS, kMaxLds / 1024);
	NR3D_CHECK(weights && packed, "mlp_pack: NULL pointer");
	NR3D_CHECK(!with_backward || nr3d_mlp_backward_packed_floats(desc) != 0, "mlp_pack: the fused backward does not apply to this network");
	PackArgs p;
	fill_layers(desc, s, false, layer_floats, p);
	for (uint32_t l = 0; l < desc->n_layers; ++l) {
		NR3D_CHECK(weights[l] != nullptr, "mlp_pack: weights[%u] is NULL", l);
		p.w[l] = weights[l];
		p.b[l] = biases ? biases[l] : nullptr;
	}
	hipLaunchKernelGGL(k_mlp_pack, dim3(16, desc->n_layers), dim3(256), 0, (hipStream_t)stream, p, packed);
	if (x3_floats(s)) {
		PackArgs x = p;
		fill_layers(desc, s, false, layer_x3_floats, x);
		hipLaunchKernelGGL(k_mlp_pack_x3, dim3(16, desc->n_layers), dim3(256), 0, (hipStream_t)stream, x, packed + packed_floats(s));
	}
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_mlp_forward(const nr3d_mlp_desc_t *desc, uint64_t n, const float *x, int64_t x_stride, int64_t x_feature_stride,
                                const float *packed, float *y, int64_t y_stride, void *stream) {
	Shape s;
	NR3D_CHECK(shape_of(desc, s) && nr3d_mlp_packed_floats(desc) != 0, "mlp_forward: network outside the fused kernels' range");
	if (n == 0) return 0;
	NR3D_CHECK(x && packed && y, "mlp_forward: NULL pointer");
	FwdArgs a;
	Layout lx, ly;
	NR3D_TRY(layout_of("mlp_forward", "x", x, x_stride, x_feature_stride, desc->dims[0], 16, lx));
	NR3D_TRY(layout_of("mlp_forward", "y", y, y_stride, 1, desc->dims[desc->n_layers], 16, ly));
	a.n = n; a.x = x; a.xs = lx.stride; a.y = y; a.ys = ly.stride; a.packed = packed;
	a.packed_floats = (uint32_t)packed_floats(s);
	const bool x3 = x3_enabled() && x3_floats(s) != 0;
	if (x3) { a.packed = packed + packed_floats(s); a.packed_floats = (uint32_t)x3_floats(s); }
	a.n_layers = desc->n_layers; a.in_dim = desc->dims[0]; a.out_dim = desc->dims[desc->n_layers];
	a.hidden_act = (int)desc->hidden_activation; a.out_act = (int)desc->output_activation;
	a.x_vec = lx.vec; a.y_vec = ly.vec;
	const size_t lds = (size_t)a.packed_floats * 4;
	const uint64_t n_tiles = (n + 31) / 32;
	const uint32_t grid = (uint32_t)(n_tiles / 4 + 1 < 1024 ? n_tiles / 4 + 1 : 1024);
	const int xf = fast_of(lx);
	int rc = 0;
	const bool sp = mlp_act::softplus_hidden(desc), sg = mlp_act::sigmoid_output(desc);
	a.beta = desc->softplus_beta;
	dispatch_tiles(s, [&](auto I, auto W, auto O) {
		constexpr int IN_T = decltype(I)::value, W_T = decltype(W)::value, OUT_T = decltype(O)::value;
		// the (bf16 route, softplus, sigmoid) variant of the tile class: the LDS limit of its three XF kernels once per device, then the launch
		auto go = [&](auto X3c, auto SPc, auto SGc) {
			constexpr bool X3 = decltype(X3c)::value, SP = decltype(SPc)::value, SG = decltype(SGc)::value;
			static LdsOnce once;
			int dev = -1;
			if ((rc = NR3D_LDS_LIMIT(once, dev, kMaxLds, k_mlp_fwd<IN_T, W_T, OUT_T, 0, X3, SP, SG>, k_mlp_fwd<IN_T, W_T, OUT_T, 1, X3, SP, SG>,
			                         k_mlp_fwd<IN_T, W_T, OUT_T, 2, X3, SP, SG>))) return;
			if (xf == 2)
				hipLaunchKernelGGL((k_mlp_fwd<IN_T, W_T, OUT_T, 2, X3, SP, SG>), dim3(grid), dim3(kThreads), lds, (hipStream_t)stream, a);
			else if (xf == 1)
				hipLaunchKernelGGL((k_mlp_fwd<IN_T, W_T, OUT_T, 1, X3, SP, SG>), dim3(grid), dim3(kThreads), lds, (hipStream_t)stream, a);
			else
				hipLaunchKernelGGL((k_mlp_fwd<IN_T, W_T, OUT_T, 0, X3, SP, SG>), dim3(grid), dim3(kThreads), lds, (hipStream_t)stream, a);
		};
		auto go_sg = [&](auto X3c, auto SPc) { if (sg) go(X3c, SPc, std::true_type{}); else go(X3c, SPc, std::false_type{}); };
		if (x3) { if (sp) go_sg(std::true_type{}, std::true_type{}); else go_sg(std::true_type{}, std::false_type{}); }
		else { if (sp) go_sg(std::false_type{}, std::true_type{}); else go_sg(std::false_type{}, std::false_type{}); }
	});
	if (rc) return rc;
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_mlp_backward(const nr3d_mlp_desc_t *desc, uint64_t n, const float *x, int64_t x_stride, int64_t x_feature_stride,
                                 const float *dL_dy, int64_t gy_stride, const float *packed, float *dL_dx, int64_t gx_stride,
                                 int64_t gx_feature_stride, float *const *dL_dW, float *const *dL_db, void *stream) {
	Shape s;
	NR3D_CHECK(shape_of(desc, s) && nr3d_mlp_backward_packed_floats(desc) != 0, "mlp_backward: the fused backward does not apply to this network");
	if (n == 0) return 0;
	NR3D_CHECK(x && dL_dy && packed && dL_dW, "mlp_backward: NULL pointer");
	BwdArgs a;
	Layout lx, lgy, lgx;
	NR3D_TRY(layout_of("mlp_backward", "x", x, x_stride, x_feature_stride, desc->dims[0], 16, lx));
	NR3D_TRY(layout_of("mlp_backward", "dL_dx", dL_dx, gx_stride, gx_feature_stride, desc->dims[0], 16, lgx));
	NR3D_TRY(layout_of("mlp_backward", "dL_dy", dL_dy, gy_stride, 1, desc->dims[desc->n_layers], 16, lgy));
	a.n = n; a.x = x; a.xs = lx.stride; a.gy = dL_dy; a.gys = lgy.stride; a.packed = packed;
	a.gx = dL_dx; a.gxs = lgx.stride;
	a.x_fm = lx.fm; a.gx_fm = lgx.fm;
	// round 6: on the bf16 MFMA with three-piece splits (forward recomputation, dH chain, dW) when the option is on and the planes fit
	const bool x3 = x3_enabled() && backward_x3(s);
	a.total_floats = (uint32_t)bwd_weight_floats(s, x3);                 // of the LDS copy (the kernel pads the packed layers itself)
	if (x3) a.packed = packed + packed_floats(s);                        // the x3 planes of the forward layers
	for (uint32_t l = 0; l < desc->n_layers; ++l) {
		NR3D_CHECK(dL_dW[l] != nullptr, "mlp_backward: dL_dW[%u] is NULL", l);
		a.dW[l] = dL_dW[l];
		a.db[l] = dL_db ? dL_db[l] : nullptr;
	}
	for (uint32_t l = 0; l <= desc->n_layers; ++l) a.dims[l] = desc->dims[l];
	a.n_layers = desc->n_layers;
	a.hidden_act = (int)desc->hidden_activation; a.out_act = (int)desc->output_activation;
	a.x_vec = lx.vec; a.gy_vec = lgy.vec; a.gx_vec = lgx.vec;
	a.tile_floats = bwd_tile_floats(s);
	a.beta = desc->softplus_beta;
	const bool sp = mlp_act::softplus_hidden(desc), sg = mlp_act::sigmoid_output(desc);
	const BwdPlan plan = bwd_plan_of(s, x3, n);
	const uint32_t nh = desc->n_layers - 1;
	const int fast = fast_of(lx, lgy);
	auto launch = [&](auto kern) -> int {
		NR3D_TRY(NR3D_LDS_LIMIT_ALWAYS(kMaxLdsBwd, kern));
		hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(64 * plan.nw), plan.lds_bytes, (hipStream_t)stream, a);
		return 0;
	};
	int rc = 0;
#define BWD_FAST(I, W, O, H, X, S, G) (fast == 2 ? launch(k_mlp_bwd<I, W, O, H, 2, X, S, G>) : fast == 1 ? launch(k_mlp_bwd<I, W, O, H, 1, X, S, G>) : launch(k_mlp_bwd<I, W, O, H, 0, X, S, G>))
#define BWD_ACT(I, W, O, H, X) (sp ? (sg ? BWD_FAST(I, W, O, H, X, true, true) : BWD_FAST(I, W, O, H, X, true, false)) \
                                   : (sg ? BWD_FAST(I, W, O, H, X, false, true) : BWD_FAST(I, W, O, H, X, false, false)))
#define BWD_CASE(I, W, O, H) if (s.in_t == I && s.w_t == W && s.out_t == O && nh == H) { \
		if (x3) { if constexpr (bwd_has_x3(I, W, O, H)) rc = BWD_ACT(I, W, O, H, true); \
		          else rc = ::nr3d::fail("mlp_backward: no bf16 MFMA backward for this shape"); } \
		else rc = BWD_ACT(I, W, O, H, false); } else
	NR3D_MLP_BWD_SHAPES(BWD_CASE)
	rc = ::nr3d::fail("mlp_backward: no kernel for this shape");
#undef BWD_CASE
#undef BWD_ACT
#undef BWD_FAST
	if (rc) return rc;
	NR3D_LAUNCH_CHECK();
	return 0;
}

// the double backward runs on every shape the fused backward runs on (same LDS plan, same waves) -- with ReLU / no hidden activation: a
// softplus network is not piecewise linear (its double backward has bias and x terms and a third chain: csrc/mlp_softplus2.hip), and
// neither is a sigmoid output (no fused double backward: a radiance decoder is differentiated once)
extern "C" int nr3d_mlp_backward_backward_ok(const nr3d_mlp_desc_t *desc) {
	return desc && !mlp_act::softplus_hidden(desc) && !mlp_act::sigmoid_output(desc) && nr3d_mlp_backward_packed_floats(desc) != 0 ? 1 : 0;
}

extern "C" int nr3d_mlp_backward_backward(const nr3d_mlp_desc_t *desc, uint64_t n, const float *x, int64_t x_stride, int64_t x_feature_stride,
                                          const float *dL_dy, int64_t gy_stride, const float *ddL_dx, int64_t v_stride,
                                          int64_t v_feature_stride, const float *packed, float *dL_ddLdy, int64_t ggy_stride,
                                          float *const *dL_dW, void *stream) {
	Shape s;
	NR3D_CHECK(!(desc && mlp_act::softplus_hidden(desc)), "mlp_backward_backward: the fused double backward does not take softplus hidden layers "
	           "(differentiate the unfused path)");
	NR3D_CHECK(!(desc && mlp_act::sigmoid_output(desc)), "mlp_backward_backward: the fused double backward does not take a sigmoid output "
	           "(differentiate the unfused path)");
	NR3D_CHECK(shape_of(desc, s) && nr3d_mlp_backward_backward_ok(desc), "mlp_backward_backward: the fused double backward does not apply to this network");
	if (n == 0) return 0;
	NR3D_CHECK(x && dL_dy && ddL_dx && packed && dL_dW, "mlp_backward_backward: NULL pointer");
	Bwd2Args a;
	Layout lx, lv, lgy, lggy;
	NR3D_TRY(layout_of("mlp_backward_backward", "x", x, x_stride, x_feature_stride, desc->dims[0], 16, lx));
	NR3D_TRY(layout_of("mlp_backward_backward", "ddL_dx", ddL_dx, v_stride, v_feature_stride, desc->dims[0], 16, lv));
	NR3D_TRY(layout_of("mlp_backward_backward", "dL_dy", dL_dy, gy_stride, 1, desc->dims[desc->n_layers], 16, lgy));
	NR3D_TRY(layout_of("mlp_backward_backward", "dL_ddLdy", dL_ddLdy, ggy_stride, 1, desc->dims[desc->n_layers], 16, lggy));
	a.n = n; a.x = x; a.xs = lx.stride; a.gy = dL_dy; a.gys = lgy.stride;
	a.v = ddL_dx; a.vs = lv.stride; a.ggy = dL_ddLdy; a.ggys = lggy.stride;
	a.x_fm = lx.fm; a.v_fm = lv.fm;
	// the route of nr3d_mlp_backward under the same option state: the masks of the forward recomputation are bit for bit its masks
	const bool x3 = x3_enabled() && backward_x3(s);
	a.packed = x3 ? packed + packed_floats(s) : packed;
	a.total_floats = (uint32_t)bwd_weight_floats(s, x3);
	for (uint32_t l = 0; l < desc->n_layers; ++l) {
		NR3D_CHECK(dL_dW[l] != nullptr, "mlp_backward_backward: dL_dW[%u] is NULL", l);
		a.dW[l] = dL_dW[l];
	}
	for (uint32_t l = 0; l <= desc->n_layers; ++l) a.dims[l] = desc->dims[l];
	a.n_layers = desc->n_layers;
	a.hidden_act = (int)desc->hidden_activation; a.out_act = (int)desc->output_activation;
	a.x_vec = lx.vec; a.v_vec = lv.vec; a.gy_vec = lgy.vec; a.ggy_vec = lggy.vec;
	a.tile_floats = bwd_tile_floats(s);
	const BwdPlan plan = bwd_plan_of(s, x3, n);
	NR3D_CHECK(plan.nw != 0, "mlp_backward_backward: no wave fits LDS");
	const uint32_t nh = desc->n_layers - 1;
	auto launch = [&](auto kern) -> int {
		NR3D_TRY(NR3D_LDS_LIMIT_ALWAYS(kMaxLdsBwd, kern));
		hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(64 * plan.nw), plan.lds_bytes, (hipStream_t)stream, a);
		return 0;
	};
	int rc = 0;
#define BWD2_CASE(I, W, O, H) if (s.in_t == I && s.w_t == W && s.out_t == O && nh == H) { \
		if (x3) { if constexpr (bwd_has_x3(I, W, O, H)) rc = launch(k_mlp_bwd2<I, W, O, H, true>); \
		          else rc = ::nr3d::fail("mlp_backward_backward: no bf16 MFMA kernel for this shape"); } \
		else rc = launch(k_mlp_bwd2<I, W, O, H>); } else
	NR3D_MLP_BWD_SHAPES(BWD2_CASE)
	rc = ::nr3d::fail("mlp_backward_backward: no kernel for this shape");
#undef BWD2_CASE
	if (rc) return rc;
	NR3D_LAUNCH_CHECK();
	return 0;
}
