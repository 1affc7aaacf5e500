// nr3d_lib_amd/csrc/importance.hip -- pixel importance sampling on accumulated error maps (models/importance.py: ErrorMap, ImpSampler;
// the reference runs all of it as chains of torch ops, nr3d_lib/models/importance.py):
//   nr3d_importance_sample         one launch: every sample of a call, for the uniform share and up to 8 maps
//   nr3d_importance_update         two launches: an accumulating, reproducible bilinear scatter of per-pixel errors into a map
//   nr3d_importance_construct_cdf  three launches: the map -> cdf_x_cond_y, cdf_y, cdf_img by wave-row scans in a fixed order
// The arithmetic is float32, one rounding per operation (this library is compiled without contraction and without fast-math; the
// divisions are IEEE), written in the order include/nr3d_hip.h states: tests/importance_ref.py restates it in numpy and the tests compare
// bytes.
//
// sample: one lane per sample.  The three searches are lower bounds (searchsorted(right=False)) with the index clamped to the row's
// last element, so that no read leaves a row whatever the row holds.
// update: launch 1 adds every contribution as a signed 64-bit fixed-point number (2^-32 units) to a scratch with an integer atomic:
// integer sums do not depend on arrival order.  Launch 2 walks the samples again, takes each touched cell out of the scratch with an
// exchange against 0 and the one lane that receives a non-zero sum adds it to the map: one writer per cell, the scratch is all zero
// again afterwards, the same bytes run after run.  (The reference's `error_map[i, h, w] += ...` is a non-accumulating index_put_: of
// two samples in one cell one survives, which one is unspecified.)
// construct_cdf: one wave per row, 64-element chunks scanned with wave_row::incl_add and a carry; no atomics.
#include "common.h"
#include "wave_row.h"

namespace nr3d {
namespace importance {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct MapTable { nr3d_importance_map_t m[NR3D_IMPORTANCE_MAX_MAPS]; };

// the first index in row[0, len) whose element is >= u, at most len - 1 (len >= 1)
__device__ __forceinline__ uint32_t lower_bound_clamped(const float *__restrict__ row, uint32_t len, float u) {
	uint32_t lo = 0, hi = len;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (row[mid] < u) lo = mid + 1; else hi = mid;
	}
	return min(lo, len - 1);
}

// the bin k of `row` that holds u and the position inside it: ((u - prev) / (row[k] - prev) + float(k)) / float(len)
__device__ __forceinline__ float invert_row(const float *__restrict__ row, uint32_t len, float u, uint32_t &k) {
	k = lower_bound_clamped(row, len, u);
	const float prev = k > 0 ? row[k - 1] : 0.0f;
	return ((u - prev) / (row[k] - prev) + (float)k) / (float)len;
}

__global__ __launch_bounds__(kBlock) void k_sample(uint32_t n, uint32_t n_images, uint32_t n_uniform, int n_maps, MapTable T,
                                                   const float *__restrict__ u_img, const float *__restrict__ u_x,
                                                   const float *__restrict__ u_y, int frame_mode, int64_t frame_const,
                                                   const int64_t *__restrict__ frame_ind, int64_t *__restrict__ out_i,
                                                   float *__restrict__ out_xy) {
	const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
	if (s >= n) return;
	// the frame: given, or drawn below
	int64_t f = frame_mode == NR3D_IMPORTANCE_FRAME_CONST ? frame_const : (frame_mode == NR3D_IMPORTANCE_FRAME_TENSOR ? frame_ind[s] : 0);
	if (f < 0) f += n_images;                              // torch's negative indices
	f = f < 0 ? 0 : (f >= (int64_t)n_images ? (int64_t)n_images - 1 : f);
	if (s < n_uniform) {
		if (frame_mode == NR3D_IMPORTANCE_FRAME_SAMPLED) {
			f = (int64_t)(u_img[s] * (float)n_images);
			if (f > (int64_t)n_images - 1) f = (int64_t)n_images - 1;
		}
		if (out_i) out_i[s] = f;
		if (out_xy) { out_xy[2 * (size_t)s] = u_x[s]; out_xy[2 * (size_t)s + 1] = u_y[s]; }
		return;
	}
	// the sample's map: the last one whose segment starts at or before s (constant indices: the table stays in scalar registers)
	nr3d_importance_map_t m = T.m[0];
#pragma unroll
	for (int k = 1; k < NR3D_IMPORTANCE_MAX_MAPS; ++k)
		if (k < n_maps && s >= T.m[k].first) m = T.m[k];
	if (frame_mode == NR3D_IMPORTANCE_FRAME_SAMPLED) f = lower_bound_clamped(m.cdf_img, n_images, u_img[s]);
	if (out_i) out_i[s] = f;
	if (!out_xy) return;
	uint32_t h, w;
	const float y = invert_row(m.cdf_y + (size_t)f * m.res_y, m.res_y, u_y[s], h);
	const float x = invert_row(m.cdf_x_cond_y + ((size_t)f * m.res_y + h) * m.res_x, m.res_x, u_x[s], w);
	out_xy[2 * (size_t)s] = x;
	out_xy[2 * (size_t)s + 1] = y;
}

// ---- update ---------------------------------------------------------------------------------------------------------------------
constexpr float kContribMax = 65536.0f;                   // 2^16: 2^15 of them fit a signed 64-bit sum of 2^-32 units
constexpr double kFixScale = 4294967296.0;                // 2^32

// one sample's four cells and contributions, as the reference's float32 expressions; false: the sample is dropped
struct Corners { size_t cell[4]; float c[4]; };
__device__ __forceinline__ bool corners(uint32_t s, uint32_t N, uint32_t H, uint32_t W, int64_t frame_const,
                                        const int64_t *__restrict__ frame_ind, const float *__restrict__ xy, const float *__restrict__ val,
                                        Corners &o) {
	const int64_t f = frame_ind ? frame_ind[s] : frame_const;
	const float x = xy[2 * (size_t)s], y = xy[2 * (size_t)s + 1], v = val[s];
	if (f < 0 || f >= (int64_t)N || !isfinite(x) || !isfinite(y) || !isfinite(v) || v < 0.0f) return false;
	const float wf = x * (float)W, hf = y * (float)H;
	if (!isfinite(wf) || !isfinite(hf)) return false;
	const float wt = truncf(wf), ht = truncf(hf);         // .long(): toward zero; float(long) is this value exactly
	const float w_w = wf - wt, w_h = hf - ht;             // BEFORE the clamp: x == 1 puts everything into column W - 2
	const uint32_t w = (uint32_t)fminf(fmaxf(wt, 0.0f), (float)(W - 2)), h = (uint32_t)fminf(fmaxf(ht, 0.0f), (float)(H - 2));
	const size_t base = ((size_t)f * H + h) * W + w;
	o.cell[0] = base;         o.c[0] = ((1.0f - w_h) * (1.0f - w_w)) * v;
	o.cell[1] = base + W;     o.c[1] = (w_h * (1.0f - w_w)) * v;
	o.cell[2] = base + 1;     o.c[2] = ((1.0f - w_h) * w_w) * v;
	o.cell[3] = base + W + 1; o.c[3] = (w_h * w_w) * v;
	return true;
}

__global__ __launch_bounds__(kBlock) void k_update_scatter(uint32_t n, uint32_t N, uint32_t H, uint32_t W, int64_t frame_const,
                                                           const int64_t *__restrict__ frame_ind, const float *__restrict__ xy,
                                                           const float *__restrict__ val, unsigned long long *__restrict__ acc) {
	const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
	if (s >= n) return;
	Corners o;
	if (!corners(s, N, H, W, frame_const, frame_ind, xy, val, o)) return;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const float c = fminf(fmaxf(o.c[k], -kContribMax), kContribMax);
		const long long q = llrint((double)c * kFixScale);
		if (q != 0) atomicAdd(&acc[o.cell[k]], (unsigned long long)q);
	}
}

__global__ __launch_bounds__(kBlock) void k_update_apply(uint32_t n, uint32_t N, uint32_t H, uint32_t W, int64_t frame_const,
                                                         const int64_t *__restrict__ frame_ind, const float *__restrict__ xy,
                                                         const float *__restrict__ val, unsigned long long *__restrict__ acc,
                                                         float *__restrict__ map) {
	const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
	if (s >= n) return;
	Corners o;
	if (!corners(s, N, H, W, frame_const, frame_ind, xy, val, o)) return;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const long long v = (long long)atomicExch(&acc[o.cell[k]], 0ull);
		if (v != 0) map[o.cell[k]] = map[o.cell[k]] + (float)((double)v * (1.0 / kFixScale));
	}
}

// ---- construct_cdf --------------------------------------------------------------------------------------------------------------
// One wave, one row: out[k] = (a * c_k) / total + b * (float(k + 1) / float(len)), c = the inclusive scan of in[k] (+ eps) in 64-element
// chunks: Kogge-Stone inside a chunk, then the carry (the previous chunk's last value, 0 before the first) added to every element.
// Returns the row total = the scan's value at the row's last element (every lane).  The unnormalised scan waits in `out`, which each lane reads back itself.
// MAP: `in` is the error map's row: e is clamped to max_pdf first (has_max), 1e-10 is added, and the clamped value (or 0: clean) goes back.
template <bool MAP>
__device__ __forceinline__ float scan_row(float *__restrict__ in, uint32_t len, float a, float b, int has_max, float max_pdf, int clean,
                                          float *__restrict__ out, int lane) {
	float carry = 0.0f;
	for (uint32_t base = 0; base < len; base += 64) {
		const uint32_t k = base + lane;
		float v = 0.0f;
		if (k < len) {
			v = in[k];
			if (MAP) {
				if (has_max && v > max_pdf) v = max_pdf;
				if (clean) in[k] = 0.0f; else if (has_max) in[k] = v;
				v = v + 1e-10f;
			}
		}
		v = wave_row::incl_add<64>(v, lane) + carry;
		carry = __shfl(v, (int)min(63u, len - 1 - base), 64);      // the chunk's last ELEMENT: lane 63, or the row's end in the last chunk
		if (k < len) out[k] = v;
	}
	const float total = carry;
	const float flen = (float)len;
	for (uint32_t k = lane; k < len; k += 64) out[k] = (a * out[k]) / total + b * ((float)(k + 1) / flen);
	return total;
}

// rows: the map [R, W] -> cdf_x_cond_y [R, W], pdf_y [R]  (R = N * H)
__global__ __launch_bounds__(kBlock) void k_cdf_rows(uint32_t R, uint32_t W, float *__restrict__ map, float a, float b, int has_max,
                                                     float max_pdf, int clean, float *__restrict__ cdf, float *__restrict__ totals) {
	const uint32_t r = blockIdx.x * kWaves + (threadIdx.x >> 6);
	if (r >= R) return;
	const int lane = threadIdx.x & 63;
	const float t = scan_row<true>(map + (size_t)r * W, W, a, b, has_max, max_pdf, clean, cdf + (size_t)r * W, lane);
	if (lane == 0) totals[r] = t;
}
// the same over rows of totals: pdf_y [N, H] -> cdf_y [N, H], pdf_img [N]; pdf_img [1, N] -> cdf_img [N]
__global__ __launch_bounds__(kBlock) void k_cdf_totals(uint32_t R, uint32_t L, float *__restrict__ in, float a, float b,
                                                       float *__restrict__ cdf, float *__restrict__ totals) {
	const uint32_t r = blockIdx.x * kWaves + (threadIdx.x >> 6);
	if (r >= R) return;
	const int lane = threadIdx.x & 63;
	const float t = scan_row<false>(in + (size_t)r * L, L, a, b, 0, 0.0f, 0, cdf + (size_t)r * L, lane);
	if (totals && lane == 0) totals[r] = t;
}

}  // namespace importance
}  // namespace nr3d

using namespace nr3d;

extern "C" int nr3d_importance_sample(uint32_t n_samples, uint32_t n_images, uint32_t n_uniform, int n_maps,
                                      const nr3d_importance_map_t *maps, const float *u_img, const float *u_x, const float *u_y,
                                      int frame_mode, int64_t frame_const, const int64_t *frame_ind, int64_t *out_i, float *out_xy,
                                      void *stream) {
	namespace im = importance;
	NR3D_CHECK(n_maps >= 0 && n_maps <= NR3D_IMPORTANCE_MAX_MAPS, "importance_sample: n_maps = %d, at most %d", n_maps, NR3D_IMPORTANCE_MAX_MAPS);
	NR3D_CHECK(frame_mode == NR3D_IMPORTANCE_FRAME_SAMPLED || frame_mode == NR3D_IMPORTANCE_FRAME_CONST ||
	           frame_mode == NR3D_IMPORTANCE_FRAME_TENSOR, "importance_sample: frame_mode = %d, must be 0 (sampled), 1 (one frame) or 2 (per sample)", frame_mode);
	NR3D_CHECK(n_uniform <= n_samples, "importance_sample: n_uniform = %u of %u samples", n_uniform, n_samples);
	if (n_samples == 0) return 0;
	NR3D_CHECK(n_images >= 1, "importance_sample: n_images = 0");
	NR3D_CHECK(n_maps >= 1 || n_uniform == n_samples, "importance_sample: %u samples beyond the uniform share and no map", n_samples - n_uniform);
	NR3D_CHECK(n_maps == 0 || maps, "importance_sample: NULL maps");
	NR3D_CHECK(out_i || out_xy, "importance_sample: neither out_i nor out_xy");
	NR3D_CHECK(frame_mode != NR3D_IMPORTANCE_FRAME_SAMPLED || u_img, "importance_sample: sampled frames without u_img");
	NR3D_CHECK(frame_mode != NR3D_IMPORTANCE_FRAME_TENSOR || frame_ind, "importance_sample: frame_mode 2 without frame_ind");
	NR3D_CHECK(frame_mode != NR3D_IMPORTANCE_FRAME_CONST || (frame_const >= -(int64_t)n_images && frame_const < (int64_t)n_images),
	           "importance_sample: frame %lld of %u images", (long long)frame_const, n_images);
	NR3D_CHECK(!out_xy || (u_x && u_y), "importance_sample: out_xy without u_x / u_y");
	im::MapTable T = {};
	for (int k = 0; k < n_maps; ++k) {
		const nr3d_importance_map_t &m = maps[k];
		NR3D_CHECK(!out_xy || (m.cdf_y && m.cdf_x_cond_y && m.res_y >= 1 && m.res_x >= 1), "importance_sample: map %d has no pixel CDFs", k);
		NR3D_CHECK(frame_mode != NR3D_IMPORTANCE_FRAME_SAMPLED || m.cdf_img, "importance_sample: map %d has no cdf_img", k);
		NR3D_CHECK(m.first >= (k ? maps[k - 1].first : n_uniform) && m.first <= n_samples && (k > 0 || m.first == n_uniform),
		           "importance_sample: map %d starts at sample %u (uniform share %u, %u samples, segments in order)", k, m.first, n_uniform, n_samples);
		T.m[k] = m;
	}
	hipLaunchKernelGGL(im::k_sample, dim3(div_up(n_samples, im::kBlock)), dim3(im::kBlock), 0, (hipStream_t)stream, n_samples, n_images,
	                   n_uniform, n_maps, T, u_img, u_x, u_y, frame_mode, frame_const, frame_ind, out_i, out_xy);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_importance_update(uint32_t n_samples, uint32_t n_images, uint32_t res_y, uint32_t res_x, int64_t frame_const,
                                      const int64_t *frame_ind, const float *xy, const float *val, float *error_map, int64_t *acc,
                                      void *stream) {
	namespace im = importance;
	NR3D_CHECK(n_samples <= NR3D_IMPORTANCE_UPDATE_CHUNK, "importance_update: %u samples, at most %u per call (a cell's 64-bit sum)", n_samples,
	           (uint32_t)NR3D_IMPORTANCE_UPDATE_CHUNK);
	NR3D_CHECK(res_y >= 2 && res_x >= 2, "importance_update: a %u x %u map has no bilinear cell", res_y, res_x);
	if (n_samples == 0 || n_images == 0) return 0;
	NR3D_CHECK(xy && val && error_map && acc, "importance_update: NULL xy, val, error_map or acc");
	hipStream_t st = (hipStream_t)stream;
	const dim3 grid(div_up(n_samples, im::kBlock)), block(im::kBlock);
	hipLaunchKernelGGL(im::k_update_scatter, grid, block, 0, st, n_samples, n_images, res_y, res_x, frame_const, frame_ind, xy, val,
	                   (unsigned long long *)acc);
	NR3D_LAUNCH_CHECK();
	hipLaunchKernelGGL(im::k_update_apply, grid, block, 0, st, n_samples, n_images, res_y, res_x, frame_const, frame_ind, xy, val,
	                   (unsigned long long *)acc, error_map);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_importance_construct_cdf(uint32_t n_images, uint32_t res_y, uint32_t res_x, float *error_map, float one_minus_min_pdf,
                                             float min_pdf, int has_max_pdf, float max_pdf, int clean, float *cdf_x_cond_y, float *cdf_y,
                                             float *cdf_img, float *pdf_y, float *pdf_img, void *stream) {
	namespace im = importance;
	NR3D_CHECK(n_images >= 1 && res_y >= 1 && res_x >= 1, "importance_construct_cdf: an empty map (%u x %u x %u)", n_images, res_y, res_x);
	NR3D_CHECK((uint64_t)n_images * res_y < (1ull << 32), "importance_construct_cdf: %u x %u rows, at most 2^32 - 1", n_images, res_y);
	NR3D_CHECK(error_map && cdf_x_cond_y && cdf_y && cdf_img && pdf_y && pdf_img, "importance_construct_cdf: NULL map, output or workspace");
	hipStream_t st = (hipStream_t)stream;
	const uint32_t R = n_images * res_y;
	hipLaunchKernelGGL(im::k_cdf_rows, dim3(div_up(R, im::kWaves)), dim3(im::kBlock), 0, st, R, res_x, error_map, one_minus_min_pdf, min_pdf,
	                   has_max_pdf, max_pdf, clean, cdf_x_cond_y, pdf_y);
	NR3D_LAUNCH_CHECK();
	hipLaunchKernelGGL(im::k_cdf_totals, dim3(div_up(n_images, im::kWaves)), dim3(im::kBlock), 0, st, n_images, res_y, pdf_y, one_minus_min_pdf,
	                   min_pdf, cdf_y, pdf_img);
	NR3D_LAUNCH_CHECK();
	hipLaunchKernelGGL(im::k_cdf_totals, dim3(1), dim3(im::kBlock), 0, st, 1u, n_images, pdf_img, one_minus_min_pdf, min_pdf, cdf_img,
	                   (float *)nullptr);
	NR3D_LAUNCH_CHECK();
	return 0;
}
