// nr3d_lib_amd/csrc/mlp_softplus2.hip -- fused fp32 decoder, double backward with softplus hidden layers (gfx950): k_mlp_bwd2_sp behind
// nr3d_mlp_softplus_backward_backward / nr3d_mlp_softplus_backward_backward_ok (ABI 21).  The eikonal term of an SDF decoder whose hidden
// activation is torch.nn.Softplus(beta, threshold = 20) -- every SDF decoder of the reference (nr3d_lib/models/fields/sdf/mlp_sdf.py:30).
// See mlp.hip for the register map and the first and second order of the ReLU / linear networks, mlp_bwd.h for what the kernels share.
#include "common.h"
#include "mlp_bwd.h"

namespace nr3d {
namespace mlp {

// =============================================================================================
// double backward with SOFTPLUS hidden layers (ABI 21).  sigma'' = beta s e is not zero (s_l = sigma'(z_l), e_l = 1 - s_l), so next to
// k_mlp_bwd2's r_l (first backward: r_L = m_L u, g_l = W_{l+1}^T r_{l+1}, r_l = s_l g_l) and t_l (tangent of v: t_0 = v,
// t_l = s_l W_l t_{l-1}) there is a third chain, hidden layers only:
//   q_l = beta e_l g_l t_l,   p_NH = q_NH,   p_l = q_l + s_l W_{l+1}^T p_{l+1},
//   dW_l = sum over samples of r_l t_{l-1}^T + p_l h_{l-1}^T (output layer: the first term),   db_l = sum of p_l,   dL/dx = W_1^T p_1,
//   dL/d(dL/dy) = m_L W_L t_NH.
// Per wave and tile of 32 samples, LDS rows X | V | G_out | H_1 .. H_NH | T_1 .. T_NH as [feature][sample]:
//   up:   layer by layer z_l = W_l h_{l-1} + b_l and W_l t_{l-1} from registers; h_l, s_l from z_l; H_l and T_l written;
//   down: one sweep that carries g_l and W_{l+1}^T p_{l+1} in registers.  At layer l every lane reads its own elements of H_l and T_l,
//         forms r_l, p_l and writes them over T_l and H_l (both dead: their last readers were layer l + 1's contractions); two
//         contractions go into the same dW accumulators, r_l with T_{l-1} and p_l with H_{l-1} (layer 1: V and X), two dense_t down.
// Where s and e come from (the second order multiplies a per-unit error by about beta): in the upward pass, and for layer NH in the
// sweep, from the pre-activation in registers with ONE exp -- E = exp(-|beta z|), the smaller of (s, e) = E / (1 + E), relative
// accuracy for dead and saturated units alike; the sign of z and that value are kept as one register per unit.  For the layers below
// NH the sweep has H_l only: e = exp(-beta h), s = 1 - e (mlp_act.h softplus_grad: <= 6e-8 absolute on s), threshold explicit.
// A padded hidden feature has s = e = 1/2 but g = t = 0 through the zero-packed weights, so r = q = p = 0 there.
// =============================================================================================
struct Bwd2SpArgs {
	uint64_t n;
	const float *x; int64_t xs;
	const float *gy; int64_t gys;
	const float *v; int64_t vs;                // dL/d(dL/dx)
	float *ggy; int64_t ggys;                  // dL/d(dL/dy) [n, out] rows; NULL: not wanted
	float *gx; int64_t gxs;                    // dL/dx; NULL: not wanted
	uint32_t x_fm, v_fm, gx_fm;                // feature-major (the stride is the feature stride)
	float beta;
	const float *packed;                       // the forward layers: f32, or their x3 planes
	uint32_t total_floats;                     // of their padded LDS copy
	uint32_t tile_floats;                      // per wave
	float *dW[NR3D_MLP_MAX_LAYERS];            // accumulated into (atomics)
	float *db[NR3D_MLP_MAX_LAYERS];            // hidden layers; may be NULL
	uint32_t dims[NR3D_MLP_MAX_LAYERS + 1];
	int out_act;
	uint32_t x_vec, gy_vec, v_vec, ggy_vec, gx_vec;
};

constexpr int kSp2MaxWaves = 4;                // 512 registers per lane: dW, g and W^T p live together

// h = softplus(z) and w = the smaller of (s, e) with the sign of z (w >= +0: s = 1 - w, e = w; w <= -0: s = -w, e = 1 + w)
__device__ __forceinline__ void softplus_hw(float z, float beta, float inv_beta, float &h, float &w) {
	const float bz = beta * z;
	const float en = __expf(-fabsf(bz)), d = 1.0f + en;
	const float m = en * __builtin_amdgcn_rcpf(d);
	const bool sat = bz > mlp_act::kSoftplusThreshold;
	h = sat ? z : fmaxf(z, 0.0f) + __logf(d) * inv_beta;
	w = sat ? 0.0f : copysignf(m, z);
}
__device__ __forceinline__ void se_of_w(float w, float &s, float &e) {
	const float m = fabsf(w), big = 1.0f - m;
	const bool neg = __builtin_bit_cast(int, w) < 0;
	s = neg ? m : big;
	e = neg ? big : m;
}
__device__ __forceinline__ void se_of_h(float h, float beta, float &s, float &e) {
	const float u = beta * h;
	const float ex = __expf(-u);
	const bool sat = u > mlp_act::kSoftplusThreshold;
	s = sat ? 1.0f : 1.0f - ex;
	e = sat ? 0.0f : ex;
}

// contract_tiles that also adds TG's sums over the samples to db (as bwd_layer: per-lane partial sums of row 32 ot + r)
template <int NO, int NI, bool X3>
__device__ __forceinline__ void contract_tiles_db(const float *__restrict__ TG, const float *__restrict__ TB, f16v (&dW)[NO][NI],
                                                  float (&db)[NO], int r, int h) {
	if constexpr (X3) {
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
}

// The pre-activations z = W hin + b of a hidden layer on the f32 route (wp: the padded f32 copy).  beta z decides s and e, and the units
// that matter to sigma'' have |z| < 0.1 while the partial sums of their dot product are of order 1: the 16-step fmaf chain of the f32
// MFMA leaves ~7e-8 absolute on such a z, which beta = 100 turns into 1e-5 of q -- 20 x torch's own fp32 error on 18 -> 32 -> 3.  So z,
// and z alone, is accumulated as dense_x3 does it: exact products of bf16 pieces, smallest terms first, summed inside the MFMA 16 at
// a time.  The weights' pieces are split here from the f32 copy (lane (i, h)'s groups 2 s and 2 s + 1 of tile (ot, it) are the eight
// values of dense_x3's A operand of step s): 24 vector instructions per operand next to 6 MFMAs of 8 passes, where the f32 MFMA
// spends 8 of 16 passes on the same 16 inputs.
template <int NI, int NO>
__device__ __forceinline__ void dense_z(const float *__restrict__ wp, const f16v (&in)[NI], f16v (&out)[NO], int lane) {
	const float *bias = wp + NO * NI * 4 * kGS;
	const int h = lane >> 5;
	const f4v *wv = reinterpret_cast<const f4v *>(wp) + h * (kHS / 4) + (lane & 31);
	constexpr bool SPLIT = (NO == 1);
	const f16v zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
	f16v alt = zero;
#pragma unroll
	for (int ot = 0; ot < NO; ++ot)
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const f4v b4 = *reinterpret_cast<const f4v *>(bias + 32 * ot + 8 * q + 4 * h);
#pragma unroll
			for (int b = 0; b < 4; ++b) out[ot][4 * q + b] = b4[b];
		}
	constexpr int PW[6] = {2, 0, 1, 1, 0, 0}, PX[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
	for (int it = 0; it < NI; ++it)
#pragma unroll
		for (int s = 0; s < 2; ++s) {
			bf8 xs[3];
			split3(in[it], s, xs);
			bf8 w[NO][3];
#pragma unroll
			for (int ot = 0; ot < NO; ++ot) {
				const f4v lo = wv[((ot * NI + it) * 4 + 2 * s) * (kGS / 4)], hi = wv[((ot * NI + it) * 4 + 2 * s + 1) * (kGS / 4)];
				split3_pair<false>(lo[0], lo[1], 0, w[ot]);
				split3_pair<false>(lo[2], lo[3], 2, w[ot]);
				split3_pair<false>(hi[0], hi[1], 4, w[ot]);
				split3_pair<false>(hi[2], hi[3], 6, w[ot]);
			}
#pragma unroll
			for (int t = 0; t < 6; ++t) {
				if constexpr (SPLIT) {
					if (t < 5) alt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0][PW[t]], xs[PX[t]], alt, 0, 0, 0);
					else out[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[0][PW[t]], xs[PX[t]], out[0], 0, 0, 0);
				} else {
#pragma unroll
					for (int ot = 0; ot < NO; ++ot) out[ot] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[ot][PW[t]], xs[PX[t]], out[ot], 0, 0, 0);
				}
			}
		}
	if constexpr (SPLIT) {
#pragma unroll
		for (int j = 0; j < 16; ++j) out[0][j] += alt[j];
	}
}

// one hidden layer of the upward pass: h = softplus(W hin + b), t = s (W tin); the (s, e) code of every unit in w
template <int NI, int NO, bool X3>
__device__ __forceinline__ void sp2_up(const float *__restrict__ wp, const f16v (&hin)[NI], const f16v (&tin)[NI], f16v (&hout)[NO],
                                       f16v (&tout)[NO], f16v (&w)[NO], float beta, float inv_beta, int lane) {
	if constexpr (X3) {
		dense_x3<NI, NO, true, true>(wp, hin, hout, NR3D_MLP_ACT_NONE, lane);
		dense_x3<NI, NO, false, true>(wp, tin, tout, NR3D_MLP_ACT_NONE, lane);
	} else {
		dense_z<NI, NO>(wp, hin, hout, lane);
		dense<NI, NO, false, true>(wp, tin, tout, NR3D_MLP_ACT_NONE, lane);
	}
#pragma unroll
	for (int t = 0; t < NO; ++t)
#pragma unroll
		for (int j = 0; j < 16; ++j) {
			float hv, wv, s, e;
			softplus_hw(hout[t][j], beta, inv_beta, hv, wv);
			se_of_w(wv, s, e);
			hout[t][j] = hv;
			w[t][j] = wv;
			tout[t][j] = s * tout[t][j];
		}
}

// one hidden layer of the downward sweep (see above).  g = W_{l+1}^T r_{l+1}, pb = W_{l+1}^T p_{l+1} (TOP: layer NH, pb is zero and
// (s, e) come from w; else from TH = H_l); TT = T_l -> r_l, TH = H_l -> p_l; TBt / TBh: the tangent / the activations of the layer's
// input; wT: the padded copy of W_l.  NEED_G / NEED_P: leave W_l^T r_l in gn / W_l^T p_l in pn.
template <int NO, int NI, bool X3, bool TOP, bool NEED_G, bool NEED_P>
__device__ __forceinline__ void sp2_down(const f16v (&g)[NO], const f16v (&pb)[NO], const f16v (&w)[NO], float beta, float *__restrict__ TT,
                                         float *__restrict__ TH, const float *__restrict__ TBt, const float *__restrict__ TBh,
                                         const float *__restrict__ wT, f16v (&dW)[NO][NI], float (&db)[NO], f16v (&gn)[NI], f16v (&pn)[NI],
                                         int lane) {
	const int r = lane & 31, h = lane >> 5;
	f16v rr[NO], pp[NO];
#pragma unroll
	for (int t = 0; t < NO; ++t)
#pragma unroll
		for (int j = 0; j < 16; ++j) {
			const int idx = (32 * t + 8 * (j >> 2) + 4 * h + (j & 3)) * kTS + r;
			float s, e;
			if constexpr (TOP) se_of_w(w[t][j], s, e);
			else se_of_h(TH[idx], beta, s, e);
			const float gv = g[t][j];
			const float q = beta * e * gv * TT[idx];
			rr[t][j] = s * gv;
			pp[t][j] = TOP ? q : q + s * pb[t][j];
		}
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	write_tile<NO>(TT, NO, rr, lane);
	write_tile<NO>(TH, NO, pp, lane);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	contract_tiles<NO, NI, X3>(TT, TBt, dW, r, h);
	contract_tiles_db<NO, NI, X3>(TH, TBh, dW, db, r, h);
	if constexpr (NEED_G) {
		if constexpr (X3) dense_x3_t<NO, NI>(wT, rr, gn, lane);
		else dense_t<NO, NI>(wT, rr, gn, lane);
	}
	if constexpr (NEED_P) {
		if constexpr (X3) dense_x3_t<NO, NI>(wT, pp, pn, lane);
		else dense_t<NO, NI>(wT, pp, pn, lane);
	}
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

template <int IN_T, int W_T, int OUT_T, int NH, bool X3 = false>
__global__ __launch_bounds__(kSp2MaxWaves * 64) void k_mlp_bwd2_sp(Bwd2SpArgs a) {
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
	const int r = lane & 31, hw = lane >> 5;
	float *tiles = lds + a.total_floats + (size_t)wave * a.tile_floats;
	// tile rows: X | V | G_out | H_1 .. H_NH | T_1 .. T_NH (sp2_tile_floats on the host side)
	float *TX = tiles;
	float *TV = TX + 32 * IN_T * kTS;
	float *TGO = TV + 32 * IN_T * kTS;
	float *TH1 = TGO + 32 * OUT_T * kTS;                                // H_l at TH1 + (l - 1) * kLT
	float *TT1 = TH1 + NH * 32 * W_T * kTS;                             // T_l at TT1 + (l - 1) * kLT
	constexpr int kLT = 32 * W_T * kTS;
	constexpr uint32_t f0 = X3 ? layer_x3_floats_pad(IN_T, W_T) : layer_floats_pad(IN_T, W_T);
	constexpr uint32_t fh = X3 ? layer_x3_floats_pad(W_T, W_T) : layer_floats_pad(W_T, W_T);
	const float *wl = lds;
	const float *wo = wl + f0 + (NH - 1) * fh;
	const float beta = a.beta, inv_beta = 1.0f / a.beta;

	f16v dW0[W_T][IN_T], dWh[NH > 1 ? NH - 1 : 1][W_T][W_T], dWo[OUT_T][W_T];
	float db0[W_T], dbh[NH > 1 ? NH - 1 : 1][W_T];
#pragma unroll
	for (int ot = 0; ot < W_T; ++ot) { zero_tiles<IN_T>(dW0[ot]); db0[ot] = 0.0f; }
#pragma unroll
	for (int l = 0; l < (NH > 1 ? NH - 1 : 1); ++l)
#pragma unroll
		for (int ot = 0; ot < W_T; ++ot) { zero_tiles<W_T>(dWh[l][ot]); dbh[l][ot] = 0.0f; }
#pragma unroll
	for (int ot = 0; ot < OUT_T; ++ot) zero_tiles<W_T>(dWo[ot]);

	const uint64_t n_tiles = (a.n + 31) / 32, step = (uint64_t)gridDim.x * nw;
	for (uint64_t tile = (uint64_t)blockIdx.x * nw + wave; tile < n_tiles; tile += step) {
		const uint64_t row = tile * 32 + r;
		const bool valid = row < a.n;
		f16v hcur[W_T], tcur[W_T], wtop[W_T], g_out[OUT_T];
		// ---- up: H_l, T_l into the tiles; x and v leave the registers after the first layer ----
		{
			f16v xin[IN_T], vin[IN_T];
			load_xv<IN_T>(a.x, a.xs, a.x_fm, a.x_vec, a.dims[0], row, a.n, lane, xin);
			load_xv<IN_T>(a.v, a.vs, a.v_fm, a.v_vec, a.dims[0], row, a.n, lane, vin);
			write_tile<IN_T>(TX, IN_T, xin, lane);
			write_tile<IN_T>(TV, IN_T, vin, lane);
			sp2_up<IN_T, W_T, X3>(wl, xin, vin, hcur, tcur, wtop, beta, inv_beta, lane);
		}
		write_tile<W_T>(TH1, W_T, hcur, lane);
		write_tile<W_T>(TT1, W_T, tcur, lane);
#pragma unroll
		for (int l = 1; l < NH; ++l) {
			f16v hn[W_T], tn[W_T];
			sp2_up<W_T, W_T, X3>(wl + f0 + (l - 1) * fh, hcur, tcur, hn, tn, wtop, beta, inv_beta, lane);
#pragma unroll
			for (int t = 0; t < W_T; ++t) { hcur[t] = hn[t]; tcur[t] = tn[t]; }
			write_tile<W_T>(TH1 + l * kLT, W_T, hcur, lane);
			write_tile<W_T>(TT1 + l * kLT, W_T, tcur, lane);
		}
		// ---- output layer: r_L = m_L u, dL/d(dL/dy) = m_L W_L t_NH ----
		load_rows<OUT_T>(a.gy, a.gys, a.dims[NH + 1], row, valid, a.gy_vec != 0, lane, g_out);     // rows past n: zero, hence every r, q, p
		uint32_t mo = ~0u;
		if (a.out_act == NR3D_MLP_ACT_RELU) {
			f16v yo[OUT_T];
			if constexpr (X3) dense_x3<W_T, OUT_T, true, true>(wo, hcur, yo, NR3D_MLP_ACT_NONE, lane);
			else dense<W_T, OUT_T, true, true>(wo, hcur, yo, NR3D_MLP_ACT_NONE, lane);
			mo = relu_bits<OUT_T>(yo);
			mask_bits<OUT_T>(g_out, mo);
		}
		if (a.ggy) {
			f16v to[OUT_T];
			if constexpr (X3) dense_x3<W_T, OUT_T, false, true>(wo, tcur, to, NR3D_MLP_ACT_NONE, lane);
			else dense<W_T, OUT_T, false, true>(wo, tcur, to, NR3D_MLP_ACT_NONE, lane);
			if (a.out_act == NR3D_MLP_ACT_RELU) mask_bits<OUT_T>(to, mo);
			store_rows<OUT_T>(a.ggy, a.ggys, a.dims[NH + 1], row, valid, a.ggy_vec != 0, lane, to);
		}
		// ---- down ----
		f16v g[W_T], pb[W_T];
		zero_tiles<W_T>(pb);
		write_tile<OUT_T>(TGO, OUT_T, g_out, lane);
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		contract_tiles<OUT_T, W_T, X3>(TGO, TT1 + (NH - 1) * kLT, dWo, r, hw);
		if constexpr (X3) dense_x3_t<OUT_T, W_T>(wo, g_out, g, lane);
		else dense_t<OUT_T, W_T>(wo, g_out, g, lane);
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
		for (int l = NH; l >= 2; --l) {                                  // hidden layer l: input H_{l-1}, T_{l-1}
			f16v gn[W_T], pn[W_T];
			float *TT = TT1 + (l - 1) * kLT, *TH = TH1 + (l - 1) * kLT;
			const float *wT = wl + f0 + (l - 2) * fh;
			if (l == NH) sp2_down<W_T, W_T, X3, true, true, true>(g, pb, wtop, beta, TT, TH, TT - kLT, TH - kLT, wT, dWh[l - 2], dbh[l - 2], gn, pn, lane);
			else sp2_down<W_T, W_T, X3, false, true, true>(g, pb, wtop, beta, TT, TH, TT - kLT, TH - kLT, wT, dWh[l - 2], dbh[l - 2], gn, pn, lane);
#pragma unroll
			for (int t = 0; t < W_T; ++t) { g[t] = gn[t]; pb[t] = pn[t]; }
		}
		f16v unused[IN_T], gx[IN_T];
		if (a.gx) {
			sp2_down<W_T, IN_T, X3, NH == 1, false, true>(g, pb, wtop, beta, TT1, TH1, TV, TX, wl, dW0, db0, unused, gx, lane);
			if (a.gx_fm) store_cols<IN_T>(a.gx, a.gxs, a.dims[0], row, valid, lane, gx);
			else store_rows<IN_T>(a.gx, a.gxs, a.dims[0], row, valid, a.gx_vec != 0, lane, gx);
		} else {
			sp2_down<W_T, IN_T, X3, NH == 1, false, false>(g, pb, wtop, beta, TT1, TH1, TV, TX, wl, dW0, db0, unused, gx, lane);
		}
	}

	// ---- reduce the waves' dW / db in LDS, one atomic per element (the output bias gets nothing) ----
	__syncthreads();
	float *R = lds + a.total_floats;
	float zbo[OUT_T];
#pragma unroll
	for (int t = 0; t < OUT_T; ++t) zbo[t] = 0.0f;
	reduce_layer<W_T, IN_T>(dW0, db0, R, a.dW[0], a.db[0], a.dims[1], a.dims[0], lane, wave, nw);
#pragma unroll
	for (int l = 1; l < NH; ++l) reduce_layer<W_T, W_T>(dWh[l - 1], dbh[l - 1], R, a.dW[l], a.db[l], a.dims[l + 1], a.dims[l], lane, wave, nw);
	reduce_layer<OUT_T, W_T>(dWo, zbo, R, a.dW[NH], nullptr, a.dims[NH + 1], a.dims[NH], lane, wave, nw);
}

}  // namespace mlp
}  // namespace nr3d

using namespace nr3d;
using namespace nr3d::mlp;

// ---- double backward with softplus hidden layers (k_mlp_bwd2_sp) ----
// per-wave tiles X | V | G_out | H_1 .. H_NH | T_1 .. T_NH: about twice k_mlp_bwd2's, so the launch has a plan of its own
static uint32_t sp2_tile_floats(const Shape &s) { return (32u * (2u * s.in_t + s.out_t) + 2u * (s.n_layers - 1) * 32u * s.w_t) * (uint32_t)kTS; }
static BwdPlan sp2_plan_of(const Shape &s, bool x3, uint64_t n = 0) {
	if (x3 && x3_floats(s) == 0) return {0, 0, 0};
	return bwd_plan(bwd_weight_floats(s, x3) * 4, (uint64_t)sp2_tile_floats(s) * 4, s.w_t, kSp2MaxWaves, 1, 0, n);
}

extern "C" int nr3d_mlp_softplus_backward_backward_ok(const nr3d_mlp_desc_t *desc) {
	Shape s;
	return desc && shape_of(desc, s) && mlp_act::softplus_hidden(desc) && !mlp_act::sigmoid_output(desc) && nr3d_mlp_backward_packed_floats(desc) != 0 &&
	       sp2_plan_of(s, false).nw != 0 ? 1 : 0;
}

extern "C" int nr3d_mlp_softplus_backward_backward(const nr3d_mlp_desc_t *desc, uint64_t n, const float *x, int64_t x_stride,
                                                   int64_t x_feature_stride, const float *dL_dy, int64_t gy_stride, const float *ddL_dx,
                                                   int64_t v_stride, int64_t v_feature_stride, const float *packed, float *dL_ddLdy,
                                                   int64_t ggy_stride, float *dL_dx, int64_t gx_stride, int64_t gx_feature_stride,
                                                   float *const *dL_dW, float *const *dL_db, void *stream) {
	Shape s;
	NR3D_CHECK(!(desc && !mlp_act::softplus_hidden(desc)), "mlp_softplus_backward_backward: softplus hidden layers only (ReLU / linear networks: "
	           "nr3d_mlp_backward_backward)");
	NR3D_CHECK(!(desc && mlp_act::sigmoid_output(desc)), "mlp_softplus_backward_backward: the fused double backward does not take a sigmoid output "
	           "(differentiate the unfused path)");
	NR3D_CHECK(shape_of(desc, s) && nr3d_mlp_softplus_backward_backward_ok(desc), "mlp_softplus_backward_backward: the fused double backward does "
	           "not apply to this network");
	if (n == 0) return 0;
	NR3D_CHECK(x && dL_dy && ddL_dx && packed && dL_dW, "mlp_softplus_backward_backward: NULL pointer");
	const char *fn = "mlp_softplus_backward_backward";
	Bwd2SpArgs a;
	Layout lx, lv, lgy, lggy, lgx;
	NR3D_TRY(layout_of(fn, "x", x, x_stride, x_feature_stride, desc->dims[0], 16, lx));
	NR3D_TRY(layout_of(fn, "ddL_dx", ddL_dx, v_stride, v_feature_stride, desc->dims[0], 16, lv));
	NR3D_TRY(layout_of(fn, "dL_dy", dL_dy, gy_stride, 1, desc->dims[desc->n_layers], 16, lgy));
	NR3D_TRY(layout_of(fn, "dL_ddLdy", dL_ddLdy, ggy_stride, 1, desc->dims[desc->n_layers], 16, lggy));
	NR3D_TRY(layout_of(fn, "dL_dx", dL_dx, gx_stride, gx_feature_stride, desc->dims[0], 16, lgx));
	a.n = n; a.x = x; a.xs = lx.stride; a.gy = dL_dy; a.gys = lgy.stride;
	a.v = ddL_dx; a.vs = lv.stride; a.ggy = dL_ddLdy; a.ggys = lggy.stride; a.gx = dL_dx; a.gxs = lgx.stride;
	a.x_fm = lx.fm; a.v_fm = lv.fm; a.gx_fm = lgx.fm;
	a.beta = desc->softplus_beta;
	// the MFMA route of nr3d_mlp_backward under the same option state, unless the bigger bf16 planes leave this kernel's tiles no wave
	const bool x3 = x3_enabled() && backward_x3(s) && sp2_plan_of(s, true).nw != 0;
	a.packed = x3 ? packed + packed_floats(s) : packed;
	a.total_floats = (uint32_t)bwd_weight_floats(s, x3);
	a.tile_floats = sp2_tile_floats(s);
	for (uint32_t l = 0; l < NR3D_MLP_MAX_LAYERS; ++l) { a.dW[l] = nullptr; a.db[l] = nullptr; }
	for (uint32_t l = 0; l < desc->n_layers; ++l) {
		NR3D_CHECK(dL_dW[l] != nullptr, "mlp_softplus_backward_backward: dL_dW[%u] is NULL", l);
		a.dW[l] = dL_dW[l];
		a.db[l] = (dL_db && l + 1 < desc->n_layers) ? dL_db[l] : nullptr;   // the output bias gets nothing
	}
	for (uint32_t l = 0; l <= desc->n_layers; ++l) a.dims[l] = desc->dims[l];
	a.out_act = (int)desc->output_activation;
	a.x_vec = lx.vec; a.gy_vec = lgy.vec; a.v_vec = lv.vec; a.ggy_vec = lggy.vec; a.gx_vec = lgx.vec;
	const BwdPlan plan = sp2_plan_of(s, x3, n);
	NR3D_CHECK(plan.nw != 0, "mlp_softplus_backward_backward: no wave fits LDS");
	const uint32_t nh = desc->n_layers - 1;
	auto launch = [&](auto kern) -> int {
		NR3D_TRY(NR3D_LDS_LIMIT_ALWAYS(kMaxLdsBwd, kern));
		hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(64 * plan.nw), plan.lds_bytes, (hipStream_t)stream, a);
		return 0;
	};
	int rc = 0;
#define BWD2SP_CASE(I, W, O, H) if (s.in_t == I && s.w_t == W && s.out_t == O && nh == H) { \
		if (x3) { if constexpr (bwd_has_x3(I, W, O, H)) rc = launch(k_mlp_bwd2_sp<I, W, O, H, true>); \
		          else rc = ::nr3d::fail("mlp_softplus_backward_backward: no bf16 MFMA kernel for this shape"); } \
		else rc = launch(k_mlp_bwd2_sp<I, W, O, H>); } else
	NR3D_MLP_BWD_SHAPES(BWD2SP_CASE)
	rc = ::nr3d::fail("mlp_softplus_backward_backward: no kernel for this shape");
#undef BWD2SP_CASE
	if (rc) return rc;
	NR3D_LAUNCH_CHECK();
	return 0;
}
