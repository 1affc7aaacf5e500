// nr3d_lib_amd/csrc/mlp_act.h -- the activations of the fused decoder beyond ReLU, shared by mlp.hip (fp32) and mlp_half.hip (half):
// the softplus HIDDEN activation (NR3D_MLP_ACT_SOFTPLUS): torch.nn.Softplus(beta, threshold = 20), the activation of the reference's SDF
// decoders (nr3d_lib/models/fields/sdf/mlp_sdf.py:30, beta = 100); and the sigmoid OUTPUT activation (NR3D_MLP_ACT_SIGMOID, below), the
// one every radiance decoder of the reference ends in (nr3d_lib/models/fields/nerf/mlp_nerf.py:196, lotd_nerf.py:219-224).
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

// which activations the fused kernels take: none / ReLU / softplus (with a beta that is finite and > 0) on the hidden layers, none /
// ReLU / sigmoid on the output layer.  Every other code -- softplus as output, sigmoid as hidden, a value outside the enum -- is refused:
// the kernels' run-time tests know these codes only and would run anything else as the identity
static inline bool softplus_hidden(const nr3d_mlp_desc_t *d) { return d->hidden_activation == NR3D_MLP_ACT_SOFTPLUS; }
static inline bool sigmoid_output(const nr3d_mlp_desc_t *d) { return d->output_activation == NR3D_MLP_ACT_SIGMOID; }
static inline bool activations_ok(const nr3d_mlp_desc_t *d) {
	const uint32_t h = d->hidden_activation, o = d->output_activation;
	if (h != NR3D_MLP_ACT_NONE && h != NR3D_MLP_ACT_RELU && h != NR3D_MLP_ACT_SOFTPLUS) return false;
	if (o != NR3D_MLP_ACT_NONE && o != NR3D_MLP_ACT_RELU && o != NR3D_MLP_ACT_SIGMOID) return false;
	if (h == NR3D_MLP_ACT_SOFTPLUS) return d->softplus_beta > 0.0f && d->softplus_beta <= 3.0e38f;   // (false for NaN)
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

// ---- the sigmoid output activation ----
// y = 1 / (1 + exp(-z)) on the fp32 accumulator z of the output layer (the half kernels: before the result is rounded to half).  With
// E = exp(-|z|) in (0, 1] and D = 1 / (1 + E) in [1/2, 1): y = D for z >= 0 and E D for z < 0, d y / dz = E D^2 -- no cancellation, so
// both tails keep their relative accuracy (the hardware exp as above: <= |z| 2^-24 + 1 ulp relative on E; the hardware reciprocal of a
// value in [1, 2]: 1 ulp, and exactly 1 for 1), and no inf * 0 for any finite z: at z = +-1e4 E is 0, y exactly 1 / 0, the derivative
// exactly 0.  The backward kernels recompute z (as they do for an output ReLU's mask) and never see a stored y.
//
// A PADDED output column (zero weights, zero bias: out_dim no multiple of 32, i.e. nearly always) holds 0.5 with derivative 0.25.
// Nothing reads it: store_rows / store_cols stop at out_dim; dL/dy is loaded as 0 beyond out_dim, or (branch-free loads) as a copy of
// real columns that meets W^T's zero rows in the dH chain -- which is what happens without an output activation too -- and the dW / db
// reductions stop at the real widths.  Rows past n of the branch-free backward paths are clamped rows (finite z) whose dL/dy was zeroed
// BEFORE it meets the derivative.
__device__ __forceinline__ float sigmoid(float z) {
	const float e = __expf(-__builtin_fabsf(z));
	const float d = __builtin_amdgcn_rcpf(1.0f + e);
	return z >= 0.0f ? d : e * d;
}
__device__ __forceinline__ float sigmoid_grad(float z) {
	const float e = __expf(-__builtin_fabsf(z));
	const float d = __builtin_amdgcn_rcpf(1.0f + e);
	return e * d * d;
}

template <int NT, class V>
__device__ __forceinline__ void sigmoid_tiles(V (&r)[NT]) {
#pragma unroll
	for (int t = 0; t < NT; ++t)
#pragma unroll
		for (int j = 0; j < 16; ++j) r[t][j] = sigmoid(r[t][j]);
}

}  // namespace mlp_act
}  // namespace nr3d
