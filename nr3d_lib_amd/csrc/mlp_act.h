// nr3d_lib_amd/csrc/mlp_act.h -- the softplus hidden activation of the fused decoder (NR3D_MLP_ACT_SOFTPLUS), shared by mlp.hip
// (fp32) and mlp_half.hip (half): torch.nn.Softplus(beta, threshold = 20), the activation of the reference's SDF decoders
// (nr3d_lib/models/fields/sdf/mlp_sdf.py:30, beta = 100).
//
// Forward, on the fp32 accumulator z of a hidden unit: h = z where beta z > 20, else log1p(exp(beta z)) / beta.
// Backward: the kernels keep every hidden layer's activations h for dW anyway, and h alone gives the derivative:
//   sigma'(z) = sigmoid(beta z) = 1 - exp(-beta h) = -expm1(-beta h)         (below the threshold: exp(beta h) = 1 + exp(beta z)),
// which is 1.0f in fp32 above the threshold (exp(-20) < 2^-25) -- torch's derivative there -- so nothing new is stored.
// No inf * 0 anywhere: beta z = 1e4 selects z (the discarded branch holds the inf), beta z = -1e4 gives exp = 0, h = 0, derivative 0.
//
// A PADDED hidden feature (zero weights, zero bias: widths that are no multiple of 32, the all-zero tile of a 3-tile width) holds
// softplus(0) = ln 2 / beta, not ReLU's 0, and derivative 1/2.  Nothing reads either: the next layer's packed weights are zero in the
// padded input columns (k_mlp_pack / k_mlp_pack_x3 / k_mlph_pack test f < in_dim, so the forward and its x3 pieces multiply it by 0
// and dL/d(padded h) = W^T dPre is 0 before it meets the derivative), and the dW / db reductions stop at the layer's real widths
// (reduce_layer / reduce_split: o < out_dim && k < in_dim).
#pragma once
#include "common.h"

namespace nr3d {
namespace mlp_act {

constexpr float kSoftplusThreshold = 20.0f;

// which activations the fused kernels take: softplus on the hidden layers only, with a beta that is finite and > 0
static inline bool softplus_hidden(const nr3d_mlp_desc_t *d) { return d->hidden_activation == NR3D_MLP_ACT_SOFTPLUS; }
static inline bool activations_ok(const nr3d_mlp_desc_t *d) {
	if (d->output_activation == NR3D_MLP_ACT_SOFTPLUS) return false;
	if (d->hidden_activation == NR3D_MLP_ACT_SOFTPLUS) return d->softplus_beta > 0.0f && d->softplus_beta <= 3.0e38f;   // (false for NaN)
	return true;
}

// The kernels around these are bound by their vector instructions (mlp_half.hip dense()), and a lane evaluates 16 units per 32-wide
// tile and layer: exp and log are the hardware's (v_exp_f32 / v_log_f32 behind __expf / __logf, ~7 instructions per unit where
// expf + log1pf take ~50).  What that costs: exp(beta z) carries a relative error of <= |beta z| 2^-24 + 1 ulp (no range reduction;
// |beta z| <= 20 here), so log(1 + e) is off by <= 1.3e-6 at the threshold, where it is 20 -- h keeps a relative error of <= 2e-7
// everywhere -- and by <= 2^-24 ABSOLUTE for beta z << 0, where h / the derivative fall below 6e-8 / beta / 6e-8 and are
// cut to 0 a little early.  Both are below one fp32 rounding of the dot product that made z.
__device__ __forceinline__ float softplus(float z, float beta, float inv_beta) {
	const float bz = beta * z;
	return bz > kSoftplusThreshold ? z : __logf(1.0f + __expf(bz)) * inv_beta;
}
// d softplus / dz from the activation h = softplus(z): -expm1(-beta h)
__device__ __forceinline__ float softplus_grad(float h, float beta) { return 1.0f - __expf(-beta * h); }

template <int NT, class V>
__device__ __forceinline__ void softplus_tiles(V (&r)[NT], float beta) {
	const float inv_beta = 1.0f / beta;
#pragma unroll
	for (int t = 0; t < NT; ++t)
#pragma unroll
		for (int j = 0; j < 16; ++j) r[t][j] = softplus(r[t][j], beta, inv_beta);
}

}  // namespace mlp_act
}  // namespace nr3d
