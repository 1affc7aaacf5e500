// nr3d_lib_amd/csrc/neus_alpha.hip -- the NeuS opacity of consecutive SDF samples, one launch each way (nr3d_neus_alpha_fwd / _bwd):
//   c_i = sigmoid(sdf_i inv_s),  alpha_i = max(0, (c_i - c_next) / (c_i + 1e-5)),
// c_next = the next sample of the same pack or row; for the last sample the appended value (1, or sigmoid(append_p inv_s)), or no
// interval at all (alpha = 0).
//
// The reference runs this as a chain of torch ops (nr3d_lib/graphics/neus/neus_utils.py:48-117: sdf * inv_s -> sigmoid -> diff |
// packed_diff -> negate -> + 1e-5 -> divide -> clamp_min: 7 launches forward and 25 backward, the backward with the reduction that
// gives a learnable inv_s its gradient; profiles/neus_alpha.json).  Here a sample is one lane's work in both directions and both layouts: the
// lane reads its own SDF value and its neighbours' and recomputes their c, so nothing crosses lanes but the sum for dL/dinv_s, and
// nothing is kept from the forward.  Packed: one wave per pack, lanes striding over it (the conventions of pack_ops.hip: my_pack,
// fill_gaps for ordered packs).  Rows: row and position from the flat sample index, no pack table.  Both call sample_alpha /
// sample_grad below, so the same data gives the same bits in either layout.
//
// A NaN in sdf gives a NaN alpha on the interval the sample opens and on the one it closes, as in the chain.  Where there is no interval
// -- the last sample of a pack without append, a row outside every pack -- the sample is not read and alpha is the 0 of the table in
// include/nr3d_hip.h, while the chain divides its 0 by sigmoid(NaN) + 1e-5 and gives NaN there (unordered packs write into a zeroed
// output: no wave owns a gap row, so it could not be otherwise).  tests/test_neus_alpha_gpu.py::test_nan pins both.
//
// dL/dinv_s = sum_i sdf_i u_i (+ the appends' terms): every workgroup writes ONE partial (lane sums, wave shuffle tree, the four waves
// added in order) into the caller's workspace, and a second launch of one workgroup adds the partials in a fixed order and WRITES the
// scalar.  No float atomics: the same bits run after run.
#include "common.h"

namespace nr3d {
namespace neus_alpha {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr float kEps = 1e-5f;

// c = sigmoid(z) and dc = c (1 - c) without cancellation (the form of mlp_act.h): E = exp(-|z|) in (0, 1], D = 1 / (1 + E);
// c = D | E D by the sign of z, dc = E D^2.  Both tails keep their relative accuracy; a NaN stays a NaN.  exp and the division are the
// accurate ones: the kernels are bound by their loads and stores, and c_i - c_next cancels whatever error c carries.
struct Cdf { float c, dc; };
__device__ __forceinline__ Cdf cdf(float z) {
	const float e = expf(-fabsf(z));
	const float d = 1.0f / (1.0f + e);
	Cdf r;
	r.c = z >= 0.0f ? d : e * d;
	r.dc = e * d * d;
	return r;
}

// one interval: q = (c - c_next) / (c + 1e-5); alpha = clamp_min(q, 0) as torch's (a NaN stays one); with the mask m = [q >= 0] (the
// gradient passes at equality, as torch's clamp_min does): a = -d alpha / d c_next = m / (c + 1e-5),
// b = d alpha / d c = m (c_next + 1e-5) / (c + 1e-5)^2
struct Interval { float alpha, a, b; };
__device__ __forceinline__ Interval interval(float c, float c_next) {
	const float den = c + kEps;
	const float q = (c - c_next) / den;
	const bool m = q >= 0.0f;
	Interval r;
	r.alpha = q < 0.0f ? 0.0f : q;
	r.a = m ? 1.0f / den : 0.0f;
	r.b = m ? (c_next + kEps) / (den * den) : 0.0f;
	return r;
}

// A segment = one pack or one row: n samples at s, the interval after the last one by `mode`.  Interval i exists for i + 1 < n and,
// with an append mode, for i = n - 1.
struct Seg { const float *s; uint32_t n; int mode; float append; };

__device__ __forceinline__ bool has_interval(const Seg &g, uint32_t i) { return i + 1 < g.n || g.mode != NR3D_NEUS_ALPHA_APPEND_NONE; }
__device__ __forceinline__ Cdf next_cdf(const Seg &g, uint32_t i, float inv_s) {
	if (i + 1 < g.n) return cdf(g.s[i + 1] * inv_s);
	if (g.mode == NR3D_NEUS_ALPHA_APPEND_ONE) { Cdf one; one.c = 1.0f; one.dc = 0.0f; return one; }
	return cdf(g.append * inv_s);
}

__device__ __forceinline__ float sample_alpha(const Seg &g, uint32_t i, float inv_s) {
	if (!has_interval(g, i)) return 0.0f;
	return interval(cdf(g.s[i] * inv_s).c, next_cdf(g, i, inv_s).c).alpha;
}

// u_i = c'_i (g_i b_i - g_{i-1} a_{i-1}): dL/dsdf_i = inv_s u_i, and sdf_i u_i is sample i's share of dL/dinv_s.  ga = dL/dalpha of the
// segment's intervals.  The previous interval is recomputed from sdf_{i-1}, so a pack longer than a wave's stride needs no carry.
__device__ __forceinline__ float sample_grad(const Seg &g, const float *__restrict__ ga, uint32_t i, float inv_s) {
	const Cdf ci = cdf(g.s[i] * inv_s);
	float t = 0.0f;
	if (has_interval(g, i)) t = ga[i] * interval(ci.c, next_cdf(g, i, inv_s).c).b;
	if (i > 0) t -= ga[i - 1] * interval(cdf(g.s[i - 1] * inv_s).c, ci.c).a;
	return ci.dc * t;
}
// the appended SDF value's own u (NR3D_NEUS_ALPHA_APPEND_SDF, n >= 1): it is c_next of the last interval only
__device__ __forceinline__ float append_grad(const Seg &g, const float *__restrict__ ga, float inv_s) {
	const Cdf ca = cdf(g.append * inv_s);
	return -(ca.dc * (ga[g.n - 1] * interval(cdf(g.s[g.n - 1] * inv_s).c, ca.c).a));
}

__device__ __forceinline__ float load_inv_s(float inv_s, const float *__restrict__ inv_s_dev) { return inv_s_dev ? inv_s_dev[0] : inv_s; }

// ---- packs: one wave per pack (pack_ops.hip's my_pack), clipped to [0, S) so that no access leaves the buffers whatever pack_infos holds
struct Pack { uint32_t p, begin, len; int lane; bool valid; };
__device__ __forceinline__ uint64_t clip_row(int64_t v, uint64_t S) { return v < 0 ? 0ull : ((uint64_t)v > S ? S : (uint64_t)v); }
__device__ __forceinline__ Pack my_pack(uint32_t P, const int64_t *__restrict__ pi, uint64_t S) {
	Pack k;
	k.lane = threadIdx.x & 63;
	k.p = blockIdx.x * kWaves + (threadIdx.x >> 6);
	k.valid = k.p < P;
	const uint64_t b = k.valid ? clip_row(pi[2 * (size_t)k.p], S) : 0ull;
	const uint64_t n = k.valid ? clip_row(pi[2 * (size_t)k.p + 1], S - b) : 0ull;
	k.begin = (uint32_t)b;
	k.len = (uint32_t)n;
	return k;
}
// ordered packs (include/nr3d_hip.h): the wave of pack p zeroes the rows up to the next pack (the last one: up to S), the wave of pack 0
// the rows in front of it
__device__ __forceinline__ void fill_gaps(const Pack &k, uint32_t P, const int64_t *__restrict__ pi, uint64_t S, float *__restrict__ out) {
	const uint64_t end = (uint64_t)k.begin + k.len;
	const uint64_t next = (k.p + 1 < P) ? clip_row(pi[2 * (size_t)(k.p + 1)], S) : S;
	for (uint64_t e = end + k.lane; e < next; e += 64) out[e] = 0.0f;
	if (k.p == 0)
		for (uint64_t e = k.lane; e < k.begin; e += 64) out[e] = 0.0f;
}
__device__ __forceinline__ Seg pack_seg(const Pack &k, const float *__restrict__ sdf, int mode, const float *__restrict__ appends) {
	Seg g;
	g.s = sdf + k.begin;
	g.n = k.len;
	g.mode = mode;
	g.append = (mode == NR3D_NEUS_ALPHA_APPEND_SDF && k.valid) ? appends[k.p] : 0.0f;
	return g;
}

__global__ __launch_bounds__(kBlock) void k_fwd_packed(uint32_t P, uint64_t S, const float *__restrict__ sdf,
                                                       const int64_t *__restrict__ pi, int mode, const float *__restrict__ appends,
                                                       float inv_s_val, const float *__restrict__ inv_s_dev, int ordered,
                                                       float *__restrict__ alpha) {
	const Pack k = my_pack(P, pi, S);
	if (!k.valid) return;
	if (ordered) fill_gaps(k, P, pi, S, alpha);
	const float inv_s = load_inv_s(inv_s_val, inv_s_dev);
	const Seg g = pack_seg(k, sdf, mode, appends);
	for (uint32_t i = k.lane; i < k.len; i += 64) alpha[k.begin + i] = sample_alpha(g, i, inv_s);
}

// rows [R, n] -> alpha [R, n_out], n_out = n - 1 (no append) or n: one lane per SAMPLE, the last one of a row without append writes nothing
__device__ __forceinline__ Seg row_seg(const float *__restrict__ sdf, uint64_t row, uint32_t n, int mode) {
	Seg g;
	g.s = sdf + row * n;
	g.n = n;
	g.mode = mode;
	g.append = 0.0f;
	return g;
}

__global__ __launch_bounds__(kBlock) void k_fwd_rows(uint64_t S, uint32_t n, const float *__restrict__ sdf, int mode, float inv_s_val,
                                                     const float *__restrict__ inv_s_dev, float *__restrict__ alpha) {
	const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
	if (e >= S) return;
	const uint32_t row = (uint32_t)e / n;                  // S < 2^32
	const uint32_t i = (uint32_t)e - row * n;
	const Seg g = row_seg(sdf, row, n, mode);
	if (!has_interval(g, i)) return;
	const uint32_t n_out = mode == NR3D_NEUS_ALPHA_APPEND_NONE ? n - 1 : n;
	alpha[(uint64_t)row * n_out + i] = sample_alpha(g, i, load_inv_s(inv_s_val, inv_s_dev));
}

// the workgroup's share of dL/dinv_s into partials[blockIdx.x]: every thread of the block calls this (no early return in front of it)
__device__ __forceinline__ void block_partial(float acc, float *__restrict__ partials) {
	__shared__ float wave_sum[kWaves];
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
	if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
	__syncthreads();
	if (threadIdx.x == 0) {
		float t = wave_sum[0];
#pragma unroll
		for (int w = 1; w < kWaves; ++w) t += wave_sum[w];
		partials[blockIdx.x] = t;
	}
}

__global__ __launch_bounds__(kBlock) void k_bwd_packed(uint32_t P, uint64_t S, const float *__restrict__ sdf,
                                                       const int64_t *__restrict__ pi, int mode, const float *__restrict__ appends,
                                                       float inv_s_val, const float *__restrict__ inv_s_dev, int ordered,
                                                       const float *__restrict__ grad_alpha, float *__restrict__ grad_sdf,
                                                       float *__restrict__ grad_appends, float *__restrict__ partials) {
	const Pack k = my_pack(P, pi, S);
	float acc = 0.0f;
	if (k.valid) {
		if (ordered) fill_gaps(k, P, pi, S, grad_sdf);
		const float inv_s = load_inv_s(inv_s_val, inv_s_dev);
		const Seg g = pack_seg(k, sdf, mode, appends);
		const float *ga = grad_alpha + k.begin;
		for (uint32_t i = k.lane; i < k.len; i += 64) {
			const float u = sample_grad(g, ga, i, inv_s);
			grad_sdf[k.begin + i] = inv_s * u;
			acc += g.s[i] * u;
		}
		if (mode == NR3D_NEUS_ALPHA_APPEND_SDF && k.lane == 0) {
			const float u = k.len ? append_grad(g, ga, inv_s) : 0.0f;
			grad_appends[k.p] = inv_s * u;
			acc += g.append * u;
		}
	}
	if (partials) block_partial(acc, partials);
}

__global__ __launch_bounds__(kBlock) void k_bwd_rows(uint64_t S, uint32_t n, const float *__restrict__ sdf, int mode, float inv_s_val,
                                                     const float *__restrict__ inv_s_dev, const float *__restrict__ grad_alpha,
                                                     float *__restrict__ grad_sdf, float *__restrict__ partials) {
	const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
	float acc = 0.0f;
	if (e < S) {
		const uint32_t row = (uint32_t)e / n;              // S < 2^32
		const uint32_t i = (uint32_t)e - row * n;
		const uint32_t n_out = mode == NR3D_NEUS_ALPHA_APPEND_NONE ? n - 1 : n;
		const float inv_s = load_inv_s(inv_s_val, inv_s_dev);
		const Seg g = row_seg(sdf, row, n, mode);
		const float u = sample_grad(g, grad_alpha + (uint64_t)row * n_out, i, inv_s);
		grad_sdf[e] = inv_s * u;
		acc = g.s[i] * u;
	}
	if (partials) block_partial(acc, partials);
}

// the partials in a fixed order: thread t adds partials[t], [t + 256], ...; then a tree over the 256 sums.  Writes, does not accumulate.
__global__ __launch_bounds__(kBlock) void k_sum_partials(uint32_t count, const float *__restrict__ partials, float *__restrict__ out) {
	__shared__ float sums[kBlock];
	float acc = 0.0f;
	for (uint32_t j = threadIdx.x; j < count; j += kBlock) acc += partials[j];
	sums[threadIdx.x] = acc;
	__syncthreads();
	for (int half = kBlock / 2; half >= 1; half >>= 1) {
		if ((int)threadIdx.x < half) sums[threadIdx.x] += sums[threadIdx.x + half];
		__syncthreads();
	}
	if (threadIdx.x == 0) out[0] = sums[0];
}

static inline uint32_t blocks_for(int layout, uint32_t P, uint64_t S) {
	return layout == NR3D_NEUS_ALPHA_PACKED ? div_up(P, kWaves) : div_up(S, kBlock);
}

// what both directions check before any launch
static int check_args(const char *fn, int layout, uint32_t P, uint64_t S, uint32_t n, const float *sdf, const int64_t *pack_infos,
                      int append_mode, const float *appends, int ordered_packs) {
	NR3D_CHECK(layout == NR3D_NEUS_ALPHA_PACKED || layout == NR3D_NEUS_ALPHA_ROWS, "%s: layout = %d, must be 0 (packed) or 1 (rows)", fn, layout);
	NR3D_CHECK(append_mode == NR3D_NEUS_ALPHA_APPEND_NONE || append_mode == NR3D_NEUS_ALPHA_APPEND_ONE ||
	           append_mode == NR3D_NEUS_ALPHA_APPEND_SDF, "%s: append_mode = %d, must be 0 (none), 1 (cdf 1) or 2 (per-pack SDF)", fn, append_mode);
	NR3D_CHECK(S < (1ull << 32), "%s: S = %llu, at most 2^32 - 1 samples per call", fn, (unsigned long long)S);
	NR3D_CHECK(S == 0 || sdf, "%s: NULL sdf", fn);
	if (layout == NR3D_NEUS_ALPHA_PACKED) {
		NR3D_CHECK(P == 0 || pack_infos, "%s: NULL pack_infos", fn);
		NR3D_CHECK(append_mode != NR3D_NEUS_ALPHA_APPEND_SDF || P == 0 || appends, "%s: append_mode 2 without pack_sdf_appends", fn);
		NR3D_CHECK(P > 0 || !ordered_packs || S == 0, "%s: ordered_packs needs at least one pack (no wave to zero the output)", fn);
	} else {
		NR3D_CHECK(n >= 1, "%s: rows of n = 0 samples", fn);
		NR3D_CHECK((uint64_t)P * n == S, "%s: rows layout with P * n = %u * %u != S = %llu", fn, P, n, (unsigned long long)S);
		NR3D_CHECK(append_mode != NR3D_NEUS_ALPHA_APPEND_SDF, "%s: per-pack SDF appends exist in the packed layout only", fn);
	}
	return 0;
}

}  // namespace neus_alpha
}  // namespace nr3d

using namespace nr3d;

extern "C" uint64_t nr3d_neus_alpha_bwd_workspace_bytes(int layout, uint32_t P, uint64_t S) {
	return (uint64_t)neus_alpha::blocks_for(layout, P, S) * sizeof(float);
}

extern "C" int nr3d_neus_alpha_fwd(int layout, uint32_t P, uint64_t S, uint32_t n, const float *sdf, const int64_t *pack_infos,
                                   int append_mode, const float *pack_sdf_appends, float inv_s, const float *inv_s_dev, int ordered_packs,
                                   float *alpha, void *stream) {
	namespace na = neus_alpha;
	NR3D_TRY(na::check_args("neus_alpha_fwd", layout, P, S, n, sdf, pack_infos, append_mode, pack_sdf_appends, ordered_packs));
	hipStream_t st = (hipStream_t)stream;
	if (layout == NR3D_NEUS_ALPHA_PACKED) {
		if (P == 0) return 0;
		NR3D_CHECK(S == 0 || alpha, "neus_alpha_fwd: NULL alpha");
		hipLaunchKernelGGL(na::k_fwd_packed, dim3(na::blocks_for(layout, P, S)), dim3(na::kBlock), 0, st, P, S, sdf, pack_infos, append_mode,
		                   pack_sdf_appends, inv_s, inv_s_dev, ordered_packs, alpha);
	} else {
		if (S == 0 || (append_mode == NR3D_NEUS_ALPHA_APPEND_NONE && n == 1)) return 0;      // no interval, no output element
		NR3D_CHECK(alpha, "neus_alpha_fwd: NULL alpha");
		hipLaunchKernelGGL(na::k_fwd_rows, dim3(na::blocks_for(layout, P, S)), dim3(na::kBlock), 0, st, S, n, sdf, append_mode, inv_s,
		                   inv_s_dev, alpha);
	}
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_neus_alpha_bwd(int layout, uint32_t P, uint64_t S, uint32_t n, const float *sdf, const int64_t *pack_infos,
                                   int append_mode, const float *pack_sdf_appends, float inv_s, const float *inv_s_dev, int ordered_packs,
                                   const float *grad_alpha, float *grad_sdf, float *grad_appends, float *grad_inv_s, void *workspace,
                                   uint64_t workspace_bytes, void *stream) {
	namespace na = neus_alpha;
	NR3D_TRY(na::check_args("neus_alpha_bwd", layout, P, S, n, sdf, pack_infos, append_mode, pack_sdf_appends, ordered_packs));
	const bool packed = layout == NR3D_NEUS_ALPHA_PACKED;
	const uint64_t n_out = packed ? S : (uint64_t)P * (append_mode == NR3D_NEUS_ALPHA_APPEND_NONE ? n - 1 : n);
	NR3D_CHECK(n_out == 0 || grad_alpha, "neus_alpha_bwd: NULL grad_alpha");
	NR3D_CHECK(S == 0 || grad_sdf, "neus_alpha_bwd: NULL grad_sdf");
	NR3D_CHECK(append_mode != NR3D_NEUS_ALPHA_APPEND_SDF || P == 0 || grad_appends, "neus_alpha_bwd: append_mode 2 without grad_appends");
	const uint32_t blocks = (packed ? P == 0 : S == 0) ? 0u : na::blocks_for(layout, P, S);
	NR3D_CHECK(!grad_inv_s || blocks == 0 || (workspace && workspace_bytes >= (uint64_t)blocks * sizeof(float)),
	           "neus_alpha_bwd: grad_inv_s needs a workspace of nr3d_neus_alpha_bwd_workspace_bytes() = %llu bytes, got %llu",
	           (unsigned long long)((uint64_t)blocks * sizeof(float)), (unsigned long long)workspace_bytes);
	hipStream_t st = (hipStream_t)stream;
	float *partials = grad_inv_s ? (float *)workspace : nullptr;
	if (blocks) {
		if (packed)
			hipLaunchKernelGGL(na::k_bwd_packed, dim3(blocks), dim3(na::kBlock), 0, st, P, S, sdf, pack_infos, append_mode, pack_sdf_appends,
			                   inv_s, inv_s_dev, ordered_packs, grad_alpha, grad_sdf, grad_appends, partials);
		else
			hipLaunchKernelGGL(na::k_bwd_rows, dim3(blocks), dim3(na::kBlock), 0, st, S, n, sdf, append_mode, inv_s, inv_s_dev, grad_alpha,
			                   grad_sdf, partials);
		NR3D_LAUNCH_CHECK();
	}
	if (grad_inv_s) {                                        // count 0: the scalar is written as 0
		hipLaunchKernelGGL(na::k_sum_partials, dim3(1), dim3(na::kBlock), 0, st, blocks, partials, grad_inv_s);
		NR3D_LAUNCH_CHECK();
	}
	return 0;
}
