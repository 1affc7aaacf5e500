// nr3d_lib_amd/csrc/permuto.hip -- host side of the permutohedral-lattice encoder: the meta builder (PermutoEncMeta::create_meta,
// csrc/permuto/src/permuto_cuda.cu:46-150) and the entry points of include/nr3d_hip.h (permuto_enc_fwd / _bwd / _bwd_bwd_input,
// permuto_cuda.cu:152-526).  The kernels are in permuto_device.h, instantiated per input dimension in permuto_d{a..g}.hip (the
// reference's compile_split_*.cu): 27 dimensions x 2 pseudo widths x 2 table dtypes x 4 kernels.
#include "permuto_device.h"
#include <math.h>
#include <string.h>

namespace nr3d {
namespace permuto {

// csrc/permuto/src/permuto_cuda.cu:44
static const int32_t kSupported[NR3D_PERMUTO_N_SUPPORTED_DIMS] = {2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20,
                                                                   24, 28, 32, 36, 40, 48, 56, 64};

static bool supported(int32_t d) {
	for (int32_t s : kSupported)
		if (s == d) return true;
	return false;
}

static DevMeta dev_meta(const nr3d_permuto_meta_t *m) {
	DevMeta d;
	memset(&d, 0, sizeof(d));
	for (uint32_t l = 0; l < m->n_levels; ++l) {
		d.level_offsets[l] = m->level_offsets[l];
		d.level_sizes[l] = m->level_sizes[l];
		d.level_n_feats[l] = m->level_n_feats[l];
		d.level_cols[l] = m->level_cols[l];
	}
	d.level_offsets[m->n_levels] = m->level_offsets[m->n_levels];
	d.n_levels = m->n_levels;
	d.n_encoded_dims = m->n_encoded_dims;
	d.n_params = m->n_params;
	return d;
}

static int run(int op, const nr3d_permuto_meta_t *meta, Args &a) {
	NR3D_CHECK(meta && supported((int32_t)meta->n_dims_to_encode), "permuto: unsupported n_dims_to_encode=%u",
	           meta ? meta->n_dims_to_encode : 0u);
	NR3D_CHECK(meta->n_levels >= 1 && meta->n_levels <= NR3D_PERMUTO_MAX_LEVELS, "permuto: bad n_levels=%u", meta->n_levels);
	NR3D_CHECK(meta->n_feat_per_pseudo_lvl == 2 || meta->n_feat_per_pseudo_lvl == 4, "permuto: n_feat_per_pseudo_lvl must be 2 or 4");
	NR3D_CHECK(a.param_dtype == NR3D_F32 || a.param_dtype == NR3D_F16, "permuto: params must be float32 or float16");
	if (a.n == 0 || a.max_level < 0) return 0;
	a.m = dev_meta(meta);
	const int D = (int)meta->n_dims_to_encode;
	const uint32_t pw = meta->n_feat_per_pseudo_lvl;
	int rc = 0;
	if (run_group_a(D, op, a, pw, &rc) || run_group_b(D, op, a, pw, &rc) || run_group_c(D, op, a, pw, &rc) ||
	    run_group_d(D, op, a, pw, &rc) || run_group_e(D, op, a, pw, &rc) || run_group_f(D, op, a, pw, &rc) ||
	    run_group_g(D, op, a, pw, &rc))
		return rc;
	return fail("permuto: no kernels for n_dims_to_encode=%d", D);
}

}  // namespace permuto
}  // namespace nr3d

using namespace nr3d;
using namespace nr3d::permuto;

extern "C" {

int nr3d_permuto_supported_n_input_dims(int32_t *dims) {
	if (dims) memcpy(dims, kSupported, sizeof(kSupported));
	return NR3D_PERMUTO_N_SUPPORTED_DIMS;
}

int nr3d_permuto_meta_create(int32_t n_input_dim, int32_t hashmap_size, uint32_t n_levels, const double *res_list,
                             const int32_t *n_feats_list, nr3d_permuto_meta_t *out, float *level_scales_multidim) {
	NR3D_CHECK(out, "permuto: NULL meta");
	memset(out, 0, sizeof(*out));
	if (!supported(n_input_dim)) {
		char list[160] = {0};
		for (int i = 0; i < NR3D_PERMUTO_N_SUPPORTED_DIMS; ++i)
			snprintf(list + strlen(list), sizeof(list) - strlen(list), i ? ",%d" : "%d", kSupported[i]);
		return fail("PermutoEncImpl: Currently not supported n_dims_to_encode=%d, while what's supported are [%s]", n_input_dim, list);
	}
	if (n_levels > NR3D_PERMUTO_MAX_LEVELS)
		return fail("PermutoEncImpl: num_level=%u exceeds maximum level=%d", n_levels, NR3D_PERMUTO_MAX_LEVELS);
	NR3D_CHECK(n_levels >= 1 && res_list && n_feats_list, "PermutoEncImpl: empty `res_list` / `n_feats_list`");
	NR3D_CHECK(hashmap_size >= 1, "PermutoEncImpl: hashmap_size=%d must be positive", hashmap_size);
	// pseudo-level width: 4 if every width divides by 4, else 2 (permuto_cuda.cu:84-94)
	bool all4 = true, all2 = true;
	for (uint32_t l = 0; l < n_levels; ++l) {
		NR3D_CHECK(n_feats_list[l] > 0, "PermutoEncImpl: n_feats_list[%u]=%d must be positive", l, n_feats_list[l]);
		all4 = all4 && n_feats_list[l] % 4 == 0;
		all2 = all2 && n_feats_list[l] % 2 == 0;
	}
	if (!all2) return fail("PermutoEncImpl: the greatest common divisor of `n_feats_list` must be at least 2");
	out->n_feat_per_pseudo_lvl = all4 ? 4 : 2;
	out->n_dims_to_encode = (uint32_t)n_input_dim;
	out->n_levels = n_levels;
	const double max_params = (double)(0xffffffffu / 2u);
	double acc_f = 0.0;
	uint32_t acc = 0, cols = 0, n_pseudo = 0;
	for (uint32_t l = 0; l < n_levels; ++l) {
		const uint32_t nf = (uint32_t)n_feats_list[l];
		out->level_n_feats[l] = nf;
		out->level_cols[l] = cols;
		cols += nf;
		n_pseudo += nf / out->n_feat_per_pseudo_lvl;
		out->level_scales0[l] = res_list[l];
		// res / sqrt((d+1)(d+2)), in double, stored as float (permuto_cuda.cu:113-116)
		for (int32_t d = 0; d < n_input_dim; ++d)
			if (level_scales_multidim)
				level_scales_multidim[l * n_input_dim + d] = (float)((double)res_list[l] / sqrt((double)(d + 1) * (d + 2)) * 1.0);
		acc_f += (double)hashmap_size * nf;
		if (acc_f > max_params) return fail("PermutoEncImpl: param size too large.");
		out->level_sizes[l] = (uint32_t)hashmap_size;
		out->level_n_params[l] = (uint32_t)hashmap_size * nf;
		out->level_offsets[l] = acc;
		acc += (uint32_t)hashmap_size * nf;
	}
	out->level_offsets[n_levels] = acc;
	out->n_params = acc;
	out->n_encoded_dims = cols;
	if (cols > 1024) return fail("PermutoEncImpl: total number of features too large. Shoule be <= 1024.");
	out->n_pseudo_levels = n_pseudo;
	uint32_t q = 0;
	for (uint32_t l = 0; l < n_levels; ++l)
		for (uint32_t j = 0; j < out->level_n_feats[l] / out->n_feat_per_pseudo_lvl; ++j, ++q) {
			out->map_levels[q] = (uint16_t)l;
			out->map_cnt[q] = (uint16_t)j;
		}
	return 0;
}

int nr3d_permuto_fwd(const nr3d_permuto_meta_t *meta, uint32_t n_points, int param_dtype, const float *x, const void *params,
                     const float *level_scales, const float *level_random_shifts, const int64_t *batch_inds,
                     const int64_t *batch_offsets, uint32_t batch_data_size, int32_t max_level, void *y, int64_t y_sn, int64_t y_se,
                     void *stream) {
	Args a = {};
	a.n = n_points; a.param_dtype = param_dtype; a.x = x; a.params = params; a.scales = level_scales; a.shifts = level_random_shifts;
	a.bidx = batch_inds; a.boffs = batch_offsets; a.bds = batch_data_size; a.max_level = max_level;
	a.y = y; a.y_sn = y_sn; a.y_se = y_se; a.st = (hipStream_t)stream;
	return run(OP_FWD, meta, a);
}

int nr3d_permuto_bwd(const nr3d_permuto_meta_t *meta, uint32_t n_points, int param_dtype, const void *dL_dy, int64_t dldy_sn,
                     int64_t dldy_se, const float *x, const void *params, const float *level_scales, const float *level_random_shifts,
                     const int64_t *batch_inds, const int64_t *batch_offsets, uint32_t batch_data_size, int32_t max_level,
                     uint32_t max_pos_dims, float *dL_dx, float *dL_dparam, void *stream) {
	Args a = {};
	a.n = n_points; a.param_dtype = param_dtype; a.x = x; a.params = params; a.scales = level_scales; a.shifts = level_random_shifts;
	a.bidx = batch_inds; a.boffs = batch_offsets; a.bds = batch_data_size; a.max_level = max_level; a.max_pos_dims = max_pos_dims;
	a.gy = dL_dy; a.gy_sn = dldy_sn; a.gy_se = dldy_se; a.dx = dL_dx; a.dp = dL_dparam; a.st = (hipStream_t)stream;
	if (dL_dx) {
		int rc = run(OP_BWD_DX, meta, a);
		if (rc) return rc;
	}
	if (dL_dparam) return run(OP_BWD_DPARAM, meta, a);
	return 0;
}

int nr3d_permuto_bwd_bwd_input(const nr3d_permuto_meta_t *meta, uint32_t n_points, int param_dtype, const float *dL_ddLdx,
                               const void *dL_dy, int64_t dldy_sn, int64_t dldy_se, const float *x, const void *params,
                               const float *level_scales, const float *level_random_shifts, const int64_t *batch_inds,
                               const int64_t *batch_offsets, uint32_t batch_data_size, int32_t max_level, void *dL_ddLdy,
                               int64_t ddldy_sn, int64_t ddldy_se, float *dL_dparam, void *stream) {
	if (!dL_ddLdy && !dL_dparam) return 0;
	Args a = {};
	a.n = n_points; a.param_dtype = param_dtype; a.x = x; a.params = params; a.scales = level_scales; a.shifts = level_random_shifts;
	a.bidx = batch_inds; a.boffs = batch_offsets; a.bds = batch_data_size; a.max_level = max_level;
	a.ggx = dL_ddLdx; a.gy = dL_dy; a.gy_sn = dldy_sn; a.gy_se = dldy_se; a.y = dL_ddLdy; a.y_sn = ddldy_sn; a.y_se = ddldy_se;
	a.dp = dL_dparam; a.st = (hipStream_t)stream;
	return run(OP_BWD_BWD, meta, a);
}

}  // extern "C"
