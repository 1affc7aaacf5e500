// nr3d_lib_amd/csrc/mlp_plan.h -- host-side plan of the fused decoder, shared by mlp.hip (fp32) and mlp_half.hip (half): which
// tile instantiation a network runs on, whether the fused backward applies, how many waves / LDS bytes / workgroups a backward
// launch gets, which layout a tensor is read in, where the layers of a pack launch start.  The kernels differ per precision
// (MFMA instruction, operand maps, LDS tiles); these facts do not, and each is stated here once.
#pragma once
#include "common.h"
#include "mlp_act.h"      // which activations the kernels take
#include <type_traits>

namespace nr3d {
namespace mlp_plan {

constexpr int kThreads = 256;                  // forward: 4 waves per workgroup, one 32-sample tile per wave at a time
constexpr int kMaxLds = 144 * 1024;            // of the CU's 160 KB
constexpr int kMaxLdsBwd = 160 * 1024;         // the backward kernels have no static LDS: the whole 160 KB

__host__ __device__ constexpr uint32_t tiles(uint32_t d) { return (d + 31u) / 32u; }

struct Shape {
	uint32_t n_layers;                         // linear layers (hidden + output)
	uint32_t in_t, w_t, out_t;                 // 32-wide tiles of the input, the (widest) hidden layer, the output
};

static bool shape_of(const nr3d_mlp_desc_t *d, Shape &s) {
	if (!d || d->n_layers < 2 || d->n_layers > NR3D_MLP_MAX_LAYERS || !mlp_act::activations_ok(d)) return false;
	uint32_t w = 0;
	for (uint32_t l = 1; l < d->n_layers; ++l) w = d->dims[l] > w ? d->dims[l] : w;
	for (uint32_t l = 0; l <= d->n_layers; ++l) if (d->dims[l] == 0 || d->dims[l] > 128) return false;
	s.n_layers = d->n_layers;
	// 3-tile widths run on the 4-tile instantiation (one all-zero tile)
	auto round = [](uint32_t t) { return t == 3 ? 4u : t; };
	s.in_t = round(tiles(d->dims[0])); s.w_t = round(tiles(w)); s.out_t = round(tiles(d->dims[d->n_layers]));
	return true;
}

// the fused backward keeps every layer's dW in accumulator registers: hidden width <= 64, at most 2 hidden layers of
// width > 32 (3 of width <= 32), input / output no wider (in tiles) than the hidden layers
static bool backward_ok(const Shape &s) {
	if (s.w_t > 2 || s.in_t > s.w_t || s.out_t > s.w_t) return false;
	const uint32_t nh = s.n_layers - 1;
	return s.w_t == 1 ? nh <= 3 : nh <= 2;
}

// f(I, W, O) with the shape's tile counts as std::integral_constant<int, 1 | 2 | 4>: the (IN_T, W_T, OUT_T) instantiation
template <class F>
static void dispatch_tiles(const Shape &s, F &&f) {
	auto pick = [](uint32_t t, auto &&g) {
		if (t == 1) g(std::integral_constant<int, 1>{});
		else if (t == 2) g(std::integral_constant<int, 2>{});
		else g(std::integral_constant<int, 4>{});
	};
	pick(s.in_t, [&](auto I) { pick(s.w_t, [&](auto W) { pick(s.out_t, [&](auto O) { f(I, W, O); }); }); });
}

// ---- backward launches ----
// Most waves a backward kernel may be launched with = its __launch_bounds__ (BwdCfg<...>::kMaxWaves) and the first count the plan tries.
// fp32: networks of 32-wide layers with <= 2 hidden layers leave room for EIGHT waves per workgroup, two per SIMD; half: every network
// of 32-wide layers (dW of such a network is <= 64 registers; the cap is then 256 per lane)
__host__ __device__ constexpr int bwd_max_waves_f32(int in_t, int w_t, int out_t, int nh) { return (in_t == 1 && w_t == 1 && out_t == 1 && nh <= 2) ? 8 : 4; }
__host__ __device__ constexpr int bwd_max_waves_half(int in_t, int w_t, int out_t) { return (in_t == 1 && w_t == 1 && out_t == 1) ? 8 : 4; }
// k_mlph_bwd_split runs with eight or four waves (eight = 256 registers per lane: only the narrow-input, narrow-output shapes stay clear
// of scratch there)
__host__ __device__ constexpr int split_max_waves(int in_t, int out_t) { return (in_t == 1 && out_t == 1) ? 8 : 4; }

// Does the fp32 backward of this shape have a bf16 ("x3") kernel?  Not the 64-wide shapes it does not win on: two hidden layers with a
// 64-wide input or output (fewer waves than the f32 copy leaves), and 64 -> 64 -> 64 (same waves, backward equal within 3 %: the splits
// of its 64-wide tiles eat what the cheaper products bring, and the f32 kernel spills less)
__host__ __device__ constexpr bool bwd_has_x3(int in_t, int w_t, int out_t, int nh) {
	return !(w_t == 2 && ((nh == 2 && in_t + out_t >= 3) || in_t + out_t >= 4));
}

// the (IN_T, W_T, OUT_T, hidden layers) instantiations of the fp32 backward, first and second order
#define NR3D_MLP_BWD_SHAPES(X) \
	X(1, 1, 1, 1) X(1, 1, 1, 2) X(1, 1, 1, 3) \
	X(1, 2, 1, 1) X(1, 2, 1, 2) X(1, 2, 2, 1) X(1, 2, 2, 2) \
	X(2, 2, 1, 1) X(2, 2, 1, 2) X(2, 2, 2, 1) X(2, 2, 2, 2)

// LDS area in which the waves' dW / db are summed, one layer at a time (it overlays the waves' tiles)
static uint64_t reduce_bytes(uint32_t w_t) { return ((uint64_t)w_t * w_t * 1024 + (uint64_t)w_t * 64) * 4; }

struct BwdPlan { uint32_t nw; size_t lds_bytes; uint32_t grid; };       // nw == 0: no wave fits LDS

// The largest wave count among nw_first, nw_first - nw_step, ... whose LDS -- the weights + max(nw tiles, reduce area) -- fits: wave
// counts above `full_lds_above` may take the whole kMaxLdsBwd, the others kMaxLds.  One workgroup per CU (dW lives in registers), each
// wave a tile of 32 samples at a time.
static BwdPlan bwd_plan(uint64_t weight_bytes, uint64_t tile_bytes, uint32_t w_t, uint32_t nw_first, uint32_t nw_step, uint32_t full_lds_above,
                        uint64_t n) {
	const uint64_t reduce = reduce_bytes(w_t);
	for (uint32_t nw = nw_first; nw >= nw_step; nw -= nw_step) {
		const uint64_t t = nw * tile_bytes, lds = weight_bytes + (t > reduce ? t : reduce);
		if (lds > (uint64_t)(nw > full_lds_above ? kMaxLdsBwd : kMaxLds)) continue;
		const uint64_t n_tiles = (n + 31) / 32;
		return {nw, (size_t)lds, (uint32_t)(n_tiles / nw + 1 < 256 ? n_tiles / nw + 1 : 256)};
	}
	return {0, 0, 0};
}

// ---- layouts ----
struct Layout {
	int64_t stride;                            // what the kernel takes: the row stride, or (fm) the feature stride
	uint32_t fm, vec;                          // feature-major; rows that can be moved in aligned pieces of 4 elements
	bool pre;                                  // vec and a width that is a multiple of 4: the branch-free (prefetching) loads apply
};

// p: [n, width] with the given strides (NULL: an output that is not wanted), align: bytes of a 4-element piece
static int layout_of(const char *fn, const char *name, const void *p, int64_t row_stride, int64_t feature_stride, uint32_t width, uint32_t align,
                     Layout &out) {
	const bool fm = p && feature_stride != 1;
	NR3D_CHECK(!fm || row_stride == 1, "%s: %s must be row-major (feature stride 1) or feature-major (row stride 1)", fn, name);
	out.stride = fm ? feature_stride : row_stride;
	out.fm = fm ? 1u : 0u;
	out.vec = (p && (uintptr_t)p % align == 0 && row_stride % 4 == 0) ? 1u : 0u;
	out.pre = out.vec && width % 4 == 0;
	return 0;
}

// the kernels' XF / FAST: 0 = any layout, 1 = prefetched row-major x, 2 = prefetched feature-major x
static int fast_of(const Layout &x) { return x.fm ? 2 : x.pre ? 1 : 0; }
// ... of a backward, which prefetches dL/dy's rows with x's
static int fast_of(const Layout &x, const Layout &gy) { return gy.pre ? fast_of(x) : 0; }

// ---- pack launches ----
// the per-layer table of a pack launch P (PackArgs of either precision): dims of W as stored, tiles of the packed layer's input / output
// (swapped when `transposed`), first element of every packed layer with layer_size(ni, no) elements per layer
template <class P, class F>
static void fill_layers(const nr3d_mlp_desc_t *d, const Shape &s, bool transposed, F layer_size, P &p) {
	p.n_layers = d->n_layers;
	uint32_t off = 0;
	for (uint32_t l = 0; l < d->n_layers; ++l) {
		p.in_dim[l] = d->dims[l]; p.out_dim[l] = d->dims[l + 1];
		const uint32_t ni = l == 0 ? s.in_t : s.w_t, no = l + 1 == d->n_layers ? s.out_t : s.w_t;
		p.ni[l] = transposed ? no : ni; p.no[l] = transposed ? ni : no;
		p.offset[l] = off;
		off += layer_size(p.ni[l], p.no[l]);
	}
	p.offset[d->n_layers] = off;
}

}  // namespace mlp_plan
}  // namespace nr3d
