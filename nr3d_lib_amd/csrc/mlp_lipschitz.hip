// nr3d_lib_amd/csrc/mlp_lipschitz.hip -- the weight normalisation of a Lipschitz MLP and its gradient, one launch each way for ALL
// layers of a network (nr3d_mlp_lipschitz_normalize / _normalize_backward).
//
// The reference's LipshitzMLP (nr3d_lib/models/blocks/mlp.py:168-249) is an ordinary MLP on normalised weights,
//   sp = softplus(c_l),  a_r = sum_j |W[r, j]|,  den_r = max(a_r, sp),  W~[r, j] = W[r, j] (sp / den_r)
// with one learnable c_l per layer, evaluated per layer and per optimiser step as abs -> sum -> softplus -> clamp_min_ -> div -> mul and
// their autograd: a chain of launches on a few KB of weights.  The samples never see the difference, so the decoder kernels (mlp.hip,
// mlp_half.hip, mlp_softplus2.hip) take W~ in place of W and nothing in them changes.
//
// A ROW is one wave's work in both directions: lanes stride over the columns, the row sums come from a fixed xor-shuffle tree, a second
// pass over the (cache-resident) row writes the result.  All arithmetic is fp32 (half weights are widened on load, W~ is rounded once to
// the weight type).  max() is written out so that a NaN propagates as torch.clamp_min does (fmaxf would drop it); softplus and its
// derivative have torch's form (beta 1, threshold 20: c > 20 -> c and 1 exactly).  Nothing else is special-cased: Inf, an all-zero row and
// an sp that underflows to 0 fall out of IEEE arithmetic, as in the torch chain.  Where a < sp the scale is sp / sp == 1 and W~ == W.
//
// Backward, with G = dL/dW~:  S_r = sum_j G[r, j] W[r, j],  q_r = sp / den_r,  pass_r = a_r >= sp (at a tie the gradient flows through a,
// as clamp_min's autograd),
//   dL/dW[r, j] = G[r, j] q_r - (pass_r ? sign(W[r, j]) S_r (q_r / den_r) : 0),      dL/dc = softplus'(c) sum_r S_r / den_r.
// The sum over the rows of a layer needs one workgroup per layer: every wave adds the terms of its rows (w, w + kWaves, ...) in order,
// the waves' sums meet in LDS and thread 0 adds them in order and WRITES dL/dc[l].  No global atomics, no zero fill, no workspace: the
// same inputs give the same bytes run after run.
#include "common.h"

namespace nr3d {
namespace lipschitz {

constexpr uint32_t kMaxLayers = NR3D_MLP_MAX_LAYERS + 1;
constexpr uint32_t kMaxDim = 4096;
constexpr int kFwdBlock = 256;                 // forward: rows are independent, 4 rows per workgroup, grid (row groups, layers)
constexpr int kBwdBlock = 1024;                // backward: ONE workgroup per layer (the row sum), so as many waves as a workgroup takes
constexpr int kBwdWaves = kBwdBlock / 64;

struct Args {
	const void *w[kMaxLayers];
	const float *g[kMaxLayers];                // backward only: dL/dW~
	void *out[kMaxLayers];                     // forward: W~ (weight type); backward: dL/dW (fp32)
	uint32_t rows[kMaxLayers], cols[kMaxLayers];
};

// torch.nn.functional.softplus(c, beta = 1, threshold = 20) and its derivative as torch's softplus_backward: z / (z + 1), z = exp(c)
__device__ __forceinline__ float softplus(float c) { return c > 20.0f ? c : log1pf(expf(c)); }
__device__ __forceinline__ float softplus_grad(float c) {
	const float z = expf(c);
	return c > 20.0f ? 1.0f : z / (z + 1.0f);
}
// torch.clamp_min(a, sp): a NaN on either side stays one
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
	return v;
}

template <typename T>
__global__ __launch_bounds__(kFwdBlock) void k_lipschitz_normalize(Args p, const float *__restrict__ c) {
	const uint32_t l = blockIdx.y;
	const uint32_t r = blockIdx.x * (kFwdBlock / 64) + (threadIdx.x >> 6);
	if (r >= p.rows[l]) return;                // (wave-uniform: the shuffles below see whole waves)
	const uint32_t cols = p.cols[l], lane = threadIdx.x & 63;
	const T *__restrict__ w = (const T *)p.w[l] + (size_t)r * cols;
	T *__restrict__ out = (T *)p.out[l] + (size_t)r * cols;
	float a = 0.0f;
	for (uint32_t j = lane; j < cols; j += 64) a += fabsf(to_f32<T>(w[j]));
	a = wave_sum(a);
	const float sp = softplus(c[l]);
	const float scale = sp / nan_max(a, sp);
	for (uint32_t j = lane; j < cols; j += 64) out[j] = from_f32<T>(to_f32<T>(w[j]) * scale);
}

template <typename T>
__global__ __launch_bounds__(kBwdBlock) void k_lipschitz_normalize_bwd(Args p, const float *__restrict__ c, float *__restrict__ dL_dc) {
	__shared__ float wave_part[kBwdWaves];
	const uint32_t l = blockIdx.x;
	const uint32_t rows = p.rows[l], cols = p.cols[l], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const float cl = c[l];
	const float sp = softplus(cl);
	float part = 0.0f;                         // sum over this wave's rows of S_r / den_r (the same value in every lane)
	for (uint32_t r = wave; r < rows; r += kBwdWaves) {
		const T *__restrict__ w = (const T *)p.w[l] + (size_t)r * cols;
		const float *__restrict__ g = p.g[l] + (size_t)r * cols;
		float *__restrict__ dw = (float *)p.out[l] + (size_t)r * cols;
		float a = 0.0f, s = 0.0f;
		for (uint32_t j = lane; j < cols; j += 64) {
			const float wj = to_f32<T>(w[j]);
			a += fabsf(wj);
			s += g[j] * wj;
		}
		a = wave_sum(a);
		s = wave_sum(s);
		const float den = nan_max(a, sp);
		const float q = sp / den;
		const bool pass = a >= sp;
		const float t = s * (q / den);
		for (uint32_t j = lane; j < cols; j += 64) {
			const float wj = to_f32<T>(w[j]);
			const float sgn = (float)((wj > 0.0f) - (wj < 0.0f));
			const float through_a = pass ? sgn * t : 0.0f;
			dw[j] = g[j] * q - through_a;
		}
		part += s / den;
	}
	if (lane == 0) wave_part[wave] = part;
	__syncthreads();
	if (threadIdx.x == 0) {
		float t = wave_part[0];
#pragma unroll
		for (int k = 1; k < kBwdWaves; ++k) t += wave_part[k];
		dL_dc[l] = softplus_grad(cl) * t;
	}
}

// what both entries check before the launch; fills the table and returns the largest row count
static int fill(const char *fn, uint32_t n_layers, const uint32_t *rows, const uint32_t *cols, const void *const *weights, const float *c,
                Args &p, uint32_t &max_rows) {
	NR3D_CHECK(n_layers >= 1 && n_layers <= kMaxLayers, "%s: n_layers = %u, must be 1..%u", fn, n_layers, kMaxLayers);
	NR3D_CHECK(rows && cols && weights && c, "%s: NULL pointer", fn);
	max_rows = 0;
	for (uint32_t l = 0; l < kMaxLayers; ++l) {
		p.w[l] = nullptr; p.g[l] = nullptr; p.out[l] = nullptr; p.rows[l] = 0; p.cols[l] = 0;
	}
	for (uint32_t l = 0; l < n_layers; ++l) {
		NR3D_CHECK(rows[l] >= 1 && cols[l] >= 1 && rows[l] <= kMaxDim && cols[l] <= kMaxDim,
		           "%s: layer %u is %u x %u, rows and columns must be 1..%u", fn, l, rows[l], cols[l], kMaxDim);
		NR3D_CHECK(weights[l] != nullptr, "%s: weights[%u] is NULL", fn, l);
		p.w[l] = weights[l]; p.rows[l] = rows[l]; p.cols[l] = cols[l];
		max_rows = rows[l] > max_rows ? rows[l] : max_rows;
	}
	return 0;
}

}  // namespace lipschitz
}  // namespace nr3d

using namespace nr3d;

extern "C" int nr3d_mlp_lipschitz_normalize(uint32_t n_layers, const uint32_t *rows, const uint32_t *cols, const void *const *weights,
                                            int weights_half, const float *c, void *const *normalized, void *stream) {
	namespace lz = lipschitz;
	lz::Args p;
	uint32_t max_rows = 0;
	NR3D_TRY(lz::fill("mlp_lipschitz_normalize", n_layers, rows, cols, weights, c, p, max_rows));
	NR3D_CHECK(normalized, "mlp_lipschitz_normalize: NULL pointer");
	for (uint32_t l = 0; l < n_layers; ++l) {
		NR3D_CHECK(normalized[l] != nullptr, "mlp_lipschitz_normalize: normalized[%u] is NULL", l);
		p.out[l] = normalized[l];
	}
	const dim3 grid(div_up(max_rows, lz::kFwdBlock / 64), n_layers);
	if (weights_half)
		hipLaunchKernelGGL(lz::k_lipschitz_normalize<__half>, grid, dim3(lz::kFwdBlock), 0, (hipStream_t)stream, p, c);
	else
		hipLaunchKernelGGL(lz::k_lipschitz_normalize<float>, grid, dim3(lz::kFwdBlock), 0, (hipStream_t)stream, p, c);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_mlp_lipschitz_normalize_backward(uint32_t n_layers, const uint32_t *rows, const uint32_t *cols,
                                                     const void *const *weights, int weights_half, const float *c,
                                                     const float *const *grads, float *const *dL_dW, float *dL_dc, void *stream) {
	namespace lz = lipschitz;
	lz::Args p;
	uint32_t max_rows = 0;
	NR3D_TRY(lz::fill("mlp_lipschitz_normalize_backward", n_layers, rows, cols, weights, c, p, max_rows));
	NR3D_CHECK(grads && dL_dW && dL_dc, "mlp_lipschitz_normalize_backward: NULL pointer");
	for (uint32_t l = 0; l < n_layers; ++l) {
		NR3D_CHECK(grads[l] != nullptr, "mlp_lipschitz_normalize_backward: grads[%u] is NULL", l);
		NR3D_CHECK(dL_dW[l] != nullptr, "mlp_lipschitz_normalize_backward: dL_dW[%u] is NULL", l);
		p.g[l] = grads[l];
		p.out[l] = dL_dW[l];
	}
	if (weights_half)
		hipLaunchKernelGGL(lz::k_lipschitz_normalize_bwd<__half>, dim3(n_layers), dim3(lz::kBwdBlock), 0, (hipStream_t)stream, p, c, dL_dc);
	else
		hipLaunchKernelGGL(lz::k_lipschitz_normalize_bwd<float>, dim3(n_layers), dim3(lz::kBwdBlock), 0, (hipStream_t)stream, p, c, dL_dc);
	NR3D_LAUNCH_CHECK();
	return 0;
}
