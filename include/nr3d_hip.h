/* include/nr3d_hip.h -- C ABI of libnr3d_hip.so (MI355X / gfx950 kernels for the nr3d hot path).
 *
 * This is the drop-in boundary: every entry point takes plain device/host pointers, sizes, element
 * strides and a hipStream_t (as void*); no torch / ATen types.  Each group cites the reference
 * interface it replaces (paths relative to the reference checkout).  All functions return 0 on
 * success, nonzero on failure with a message available from nr3d_last_error() (thread-local).
 *
 * Ownership: the CALLER allocates every buffer (inputs and outputs) on the device the stream
 * belongs to; the library holds no state besides the thread-local error string and the option table below.  Buffers documented
 * "zero-init" must be zeroed by the caller; all other outputs are fully written by the kernels
 * (skipped points are written as zeros), so they may be allocated uninitialised.
 *
 * dtype codes (NR3D_*) name the element type behind a void*.
 */
#ifndef NR3D_HIP_H
#define NR3D_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { NR3D_F32 = 0, NR3D_F16 = 1, NR3D_F64 = 2, NR3D_I32 = 3, NR3D_I64 = 4, NR3D_U8 = 5, NR3D_I16 = 6, NR3D_I8 = 7 };

/* Bumped whenever an entry point is removed or changes its parameters, or an addition touches an existing one.  An addition that leaves
 * every existing entry untouched keeps the number (nr3d_marching_cubes_*, nr3d_knn_*, nr3d_forest_ray_test_*): the Python loader refuses, by name, a library that lacks an
 * entry its table declares (_hip._declare), so an older build behind newer bindings is still an error at load.  nr3d_lib_amd/_abi.py
 * (generated from this header by tools/gen_abi.py at build time) carries the same number next to every entry point's argument types;
 * the loader also refuses a library whose nr3d_abi_version() differs, so a vendored nr3d_lib_amd/ needs this header neither at import
 * nor at run time. */
#define NR3D_ABI_VERSION 30

const char *nr3d_last_error(void);
int nr3d_abi_version(void);

/* Optional per-kernel timing with HIP events on the launch stream (what the reference's c_profile flag does for whole
 * calls: csrc/lotd/include/lotd/lotd_hash_only.h:748-760, LoDMeta::c_profile lotd_torch_api.h:102-110).
 * nr3d_prof_enable(mask): bit id set => every launch of that kernel is bracketed by an event pair (off: no cost).
 * nr3d_prof_read: sum of the recorded intervals of `id` in ms and their number (synchronises on them); reset != 0
 * forgets them.  Used by bench.py for `roofline.achieved` of the dominant kernel. */
enum {
	NR3D_PROF_LOTD_FWD = 0,          /* k_fwd: forward of all levels served from L2 */
	NR3D_PROF_LOTD_FWD_LDS = 1,      /* k_fwd_lds: forward of the levels staged in LDS (one interval per level) */
	NR3D_PROF_LOTD_CONTRACT_DX = 2,  /* dL/dx = dL/dy . dy/dx */
	NR3D_PROF_LOTD_BIN = 3,          /* dL/dparam stage A */
	NR3D_PROF_LOTD_ACCUM = 4,        /* dL/dparam stage B */
	NR3D_PROF_MARCH = 5,             /* ray marching, count + emit */
	NR3D_PROF_COMPOSITE_FWD = 6,     /* fused alpha composite */
	NR3D_PROF_COMPOSITE_BWD = 7,
	NR3D_PROF_LOTD_DIRECT = 8,       /* dL/dparam of the levels that skip the records (k_pair_direct) */
	NR3D_PROF_COUNT = 9
};
void nr3d_prof_enable(uint32_t mask);
int nr3d_prof_read(int id, double *total_ms, uint32_t *n_intervals, int reset);

/* Selectable code paths (round 4: ONE table instead of environment switches; no launch reads the environment).
 * Every entry chooses between two implementations of the SAME result -- the parity tests run both and compare them with
 * each other and with the oracle -- so a caller never needs them; they exist for A/B measurement and cross-checks.
 * nr3d_set_option(id, value): value < 0 restores the default; returns nonzero for an unknown id.  nr3d_get_option: current value,
 * -1 if unknown.
 * TEST / MEASUREMENT ONLY -- not part of the drop-in surface.  The table is process-wide on purpose (an option set on the Python main
 * thread has to reach the launches PyTorch's autograd engine issues from ITS device thread, which a thread-local table would not);
 * entries are relaxed atomics, so a concurrent set/launch is not a data race, but two host threads that A/B DIFFERENT values at the
 * same time see each other's choice -- results stay correct (both implementations give the same result), measurements do not.
 * Production callers never set one: every default is the measured-fastest path.
 * The library has no build-time variants and reads nothing from the environment; the timing decompositions of the past are
 * recorded under profiles/. */
enum {
	NR3D_OPT_LOTD_PAIR = 0,          /* 1: pair / quad records for dL/dparam of 3-D Dense/Hash metas (lotd_pair.hip); 0: corner records */
	NR3D_OPT_PAIR_QUAD = 1,          /* 1: Dense levels of the pair path as quad records */
	NR3D_OPT_PAIR_SECOND = 2,        /* 1: d(dL/dx)/dparam of pair-path metas on pair records */
	NR3D_OPT_PAIR_DIRECT = 3,        /* 1: levels with <= 4 buckets skip the records (k_pair_direct) */
	NR3D_OPT_PAIR_FIXED = 4,         /* 1: 64-bit fixed-point LDS accumulators; 0: fp64 */
	NR3D_OPT_FWD_PAIRLANE = 5,       /* 1: two-lane forward / Hessian kernels for 3-D Dense/Hash metas; 0: k_fwd (corner sum) */
	NR3D_OPT_FWD_SPLIT = 6,          /* 1: mixed metas launch per level type */
	NR3D_OPT_FWD_LDS_STAGE = 7,      /* 1: coarse Dense levels whose whole table fits LDS are served from it (k_fwd_lds); 0: none */
	NR3D_OPT_HVP_LEVELS = 8,         /* 1: d(dL/dx)/dx with one lane per (point, level) when a workspace is given */
	NR3D_OPT_HVP_PAIRLANE = 9,       /* 1: ... through the two-lane gather */
	NR3D_OPT_HVP_SPLIT = 10,         /* 1: lane-serial d(dL/dx)/dx launches per level type */
	NR3D_OPT_VM_SPLIT = 11,          /* 1: stage A of VM levels with three threads per point */
	NR3D_OPT_CP_DIRECT = 12,         /* 1: CP levels' dL/dparam accumulated in LDS without records */
	NR3D_OPT_MARCH_GROUP = 13,       /* 0: lanes per ray chosen from the ray count; 1 | 16 | 32 | 64 forces */
	NR3D_OPT_PACK_SCAN = 14,         /* 1: fused composite on wave prefix products; 0: serial replay */
	NR3D_OPT_SORT_WAVE = 15,         /* 1: packed_sort with one wave per pack (bitonic); 0: one lane per pack (heapsort) */
	NR3D_OPT_VM_DIRECT = 16,         /* 1: VM levels whose planes split into <= 4 LDS-sized bands accumulate their dL/dparam in LDS without records (k_vm_direct) */
	NR3D_OPT_DIRECT_FIXED = 17,      /* 1: k_cp_direct and k_vm_sorted accumulate in 64-bit fixed point (scale from the workgroup's own bound on its updates); 0: fp64 */
	NR3D_OPT_VM_SORTED = 18,         /* 1: a dL/dparam pass with a VM level of >= 2^20 entries (over its blocks) and >= 2^19 points -- or any VM level and >= 2^21 points -- sorts the POINTS by
	                                  * (block, coordinate) and accumulates every VM level band by band in LDS, without records (lotd_sorted.hip;
	                                  * single tables, batches and forests; a forest's small Dense levels ride along as slices); 2: whenever the geometry allows (tests); 3: as 1, VM levels only; 0: records */
	NR3D_OPT_MLP_X3 = 19,            /* 1: the fp32 fused MLP forward runs on the bf16 MFMA with every value split into three bf16 pieces (six piece products,
	                                  * fp32 accumulation: fp32-grade results at 2.7x the matrix rate of the f32 MFMA); 0: v_mfma_f32_32x32x2_f32.
	                                  * Non-finite inputs: a row holding +-inf (or a magnitude above the bf16 maximum, 3.39e38) comes out as NaN on the
	                                  * x3 route (inf - bf16(inf) = NaN in the split) where the f32 MFMA gives +-inf or NaN (inf * 0); finite rows of the
	                                  * same batch are unaffected on both.  A ReLU pre-activation within ~1 ulp of zero may be masked differently by a
	                                  * forward on one route and a backward recomputation on the other (the gradient of that unit at that sample only). */
	NR3D_OPT_PAIR_FOLD = 20,         /* 1: a dL/dparam call on the pair path that follows nr3d_lotd_bwd_dx (with `fold`) takes the fixed-point scale from that kernel and
	                                  * runs as stage A, k_pair_direct (with the replica plan folded in) and stage B (with the replica sums folded in); 0: the
	                                  * separate gmax fill, k_pair_plan and k_pair_reduce launches */
	NR3D_OPT_COUNT = 21
};
int nr3d_set_option(int id, int64_t value);
int64_t nr3d_get_option(int id);

/* =================================================================================================
 * LoTD encoder -- replaces nr3d_lib.bindings._lotd
 *   pybind surface   csrc/lotd/src/lotd.cpp:23-110
 *   host API         csrc/lotd/include/lotd/lotd_torch_api.h:79-249, csrc/lotd/src/lotd_torch_api.cu
 *   device meta      csrc/lotd/include/lotd/lotd_cuda.h:29-76 (LoDMetaRef)
 * ============================================================================================== */
#define NR3D_LOTD_MAX_LEVELS 32
#define NR3D_LOTD_MAX_DIMS 4
#define NR3D_LOTD_MAX_PSEUDO 256

/* csrc/lotd/include/lotd/lotd_types.h:16-25 */
enum {
	NR3D_LOD_Dense = 0, NR3D_LOD_VectorMatrix = 1, NR3D_LOD_VecZMatXoY = 2, NR3D_LOD_CP = 3,
	NR3D_LOD_CPfast = 4, NR3D_LOD_NPlaneMul = 5, NR3D_LOD_NPlaneSum = 6, NR3D_LOD_Hash = 7
};

typedef struct nr3d_lotd_level {
	uint32_t res[NR3D_LOTD_MAX_DIMS]; /* level_res_multidim */
	uint32_t n_feats;                 /* level_n_feats  */
	uint32_t type;                    /* level_types    */
	uint32_t size;                    /* level_sizes    (entries, feature width not counted) */
	uint32_t offset;                  /* level_offsets  (elements, inside one batch entry)   */
} nr3d_lotd_level_t;                  /* 32 B: one level per half cache line */

typedef struct nr3d_lotd_meta {
	nr3d_lotd_level_t levels[NR3D_LOTD_MAX_LEVELS];
	uint16_t map_levels[NR3D_LOTD_MAX_PSEUDO];
	uint16_t map_cnt[NR3D_LOTD_MAX_PSEUDO];
	uint32_t n_levels;
	uint32_t n_pseudo_levels;
	uint32_t n_feat_per_pseudo_lvl;
	uint32_t n_dims_to_encode;
	uint32_t n_encoded_dims;
	uint32_t n_params;               /* == level_offsets[n_levels] */
	uint32_t interpolation_type;     /* 0 Linear, 1 Smoothstep (lotd_types.h:78-82) */
	uint32_t c_hash_only;            /* every level is Dense or Hash */
	/* ABI 2 (appended; everything above is unchanged): first output column of pseudo level q.  q * n_feat_per_pseudo_lvl
	 * for the meta nr3d_lotd_meta_create builds; a REGROUPED meta (nr3d_lotd_meta_regroup) lists a subset of the levels with
	 * a wider pseudo level, and its columns are those of the original layout. */
	uint16_t map_col[NR3D_LOTD_MAX_PSEUDO];
} nr3d_lotd_meta_t;

/* LoDMeta::create_meta (lotd_torch_api.cu:29-230).  Host only, no GPU needed.
 * res_multidim is [n_levels, n_input_dim] row-major; types are NR3D_LOD_* codes. */
int nr3d_lotd_meta_create(int32_t n_input_dim, uint32_t n_levels, const int32_t *res_multidim,
                          const int32_t *n_feats, const int32_t *types, uint32_t hashmap_size,
                          int use_smooth_step, nr3d_lotd_meta_t *out);

/* Pseudo levels regrouped by feature width (no reference counterpart: the reference processes every level in pseudo levels
 * of the GLOBAL gcd of the widths, lotd_torch_api.cu:58-75 -- a meta that mixes 2- and 16-feature levels walks the
 * 16-feature one as eight 2-feature pseudo levels, repeating the index work eight times).  *out = *meta with
 * n_feat_per_pseudo_lvl = width (2, 4 or 8) and ONLY the pseudo levels of the levels whose own widest admissible width
 * (largest of 8, 4, 2 dividing n_feats, capped at `max_width`) is `width`; levels, offsets, n_encoded_dims and the output columns (map_col) are
 * those of *meta, so calls with the regrouped metas of all three widths write disjoint columns / table slices of the same
 * tensors and together equal one call with *meta.  out->n_pseudo_levels == 0: no level has that width. */
int nr3d_lotd_meta_regroup(const nr3d_lotd_meta_t *meta, uint32_t width, uint32_t max_width, nr3d_lotd_meta_t *out);

/* Batch addressing shared by all LoTD entry points (lotd_encoding.h:166-178):
 *   batch_inds   int64 [N] or NULL (value < 0 => point skipped)
 *   batch_offsets int64 [B] or NULL (element offset of each batch entry; default b * n_params)
 *   batch_data_size  >0 => b = i / batch_data_size when batch_inds is NULL
 *   max_level    levels > max_level contribute zeros; <= -1 => everything zero (lotd_torch_api.cu:294)
 * `meta_dev` is a device-resident byte copy of *meta (the caller uploads it once per meta/device).
 * Strides are in ELEMENTS.  x is [N, D] contiguous; params is 1-D contiguous.
 * param_dtype: NR3D_F32, or NR3D_F16 -- `params` are __half tables, read as half and used as float (the reference's
 * (float, half, float) dispatch, lotd_encoding.h:1501-1504) by every kernel that reads table entries: every meta, batched
 * tables and (ABI 3) the forest entry points included; a half table gives bit for bit what its fp32 copy gives.  With NR3D_F16 nr3d_lotd_fwd writes y as __half
 * (the fp32 result rounded once); dy_dx and dL_dx stay float, and so do dL_dy and dL_dparam
 * except where nr3d_lotd_half_params_ok says that nr3d_lotd_bwd_dparam takes them as __half (grad_dtype / out_dtype).
 */

/* lod_fwd (lotd_torch_api.cu:232-395): y[i*y_sn + e*y_se] (params dtype);
 * dy_dx[i*dydx_sn + e*dydx_se + d] (x dtype) or NULL. */
int nr3d_lotd_fwd(const nr3d_lotd_meta_t *meta, const void *meta_dev, uint32_t n_points,
                  int x_dtype, int param_dtype, const void *x, const void *params,
                  const int64_t *batch_inds, const int64_t *batch_offsets, uint32_t batch_data_size,
                  int32_t max_level, void *y, int64_t y_sn, int64_t y_se,
                  void *dy_dx, int64_t dydx_sn, int64_t dydx_se, void *stream);

/* lod_bwd, input-gradient half (lotd_encoding.h:1562-1586 / lotd_hash_only.h:839-863):
 * dL_dx[i, d] = sum_e dL_dy[i, e] * dy_dx[i, e, d];  dL_dx is [N, D] contiguous (x dtype). */
int nr3d_lotd_bwd_dx(const nr3d_lotd_meta_t *meta, uint32_t n_points, int x_dtype, int param_dtype,
                     const void *dL_dy, int64_t dldy_sn, int64_t dldy_se,
                     const void *dy_dx, int64_t dydx_sn, int64_t dydx_se, void *dL_dx,
                     void *dL_dy_T /* optional out, f32 [n_encoded_dims, n_points]: feature-major copy of a contiguous
                                      dL_dy; pass it to nr3d_lotd_bwd_dparam as dL_dy with strides (1, n_points) and
                                      the scatter skips its own transposition */,
                     int32_t max_level, void *fold /* optional out, the hand-over buffer of the folded pair path (see
                                      nr3d_lotd_bwd_dparam below); NULL: max_level is not used */,
                     void *stream);

/* Scratch of nr3d_lotd_bwd_dparam's atomic-free routes for n_points points and n_batches table sets; 0: they do not serve this
 * meta (4-D NPlaneMul / NPlaneSum levels). */
uint64_t nr3d_lotd_dparam_workspace_bytes(const nr3d_lotd_meta_t *meta, uint32_t n_points, uint32_t n_batches);
/* Tuning knob: points per pass of the atomic-free scatter = 2^log2_points (10..24; 0 restores the default 2^22 or
 * NR3D_LOTD_BIN_CHUNK_LOG2).  The workspace size follows; query it again after changing this. */
void nr3d_lotd_set_dparam_chunk_log2(int log2_points);

/* dL_dy [N, E] (element (i, e) at i * g_sn + e * g_se; grad_dtype NR3D_F32 | NR3D_F16) -> out float [E][N], feature-major:
 * the layout the level-major kernels read.  nr3d_lotd_bwd_dparam makes this copy itself when handed a row-major dL_dy; a caller
 * that runs several entries on one dL_dy (d(dL/dx)/dparam and d(dL/dx)/dx of one second-order step) makes it once and passes it
 * with strides (1, N) to nr3d_lotd_bwd_dparam and nr3d_lotd_bwd_bwd_dx. */
int nr3d_lotd_dLdy_feature_major(uint32_t n_points, uint32_t n_encoded_dims, int grad_dtype, const void *dL_dy,
                                 int64_t g_sn, int64_t g_se, float *out, void *stream);

/* Native half-parameter storage, the reference's (float, half, float) type combination (<input, param, compute>,
 * csrc/lotd/include/lotd/lotd_encoding.h:1501-1504; PARAM_T accumulators lotd_encoding.h:72): x and dy_dx float, params /
 * y / dL_dy / dL_dparam __half, arithmetic in fp32.  1 when nr3d_lotd_fwd (param_dtype NR3D_F16: y is __half too),
 * nr3d_lotd_bwd_dx (param_dtype NR3D_F16: dL_dy is __half, contiguous [N, E]) and nr3d_lotd_bwd_dparam (grad_dtype / out_dtype
 * NR3D_F16) serve this meta with half GRADIENTS as well -- unbatched 3-D Dense/Hash metas with 2-feature pseudo levels; for every
 * other meta the half TABLES are still read as they are (param_dtype above) and only dL_dy / dL_dparam pass through float.
 * Unlike the reference's __half2 atomics the parameter gradient is accumulated exactly and rounded to half once. */
int nr3d_lotd_half_params_ok(const nr3d_lotd_meta_t *meta, int batched);
/* 1 when an unbatched nr3d_lotd_bwd_dparam call with a workspace takes the pair-record path for this meta (3-D Dense/Hash
 * levels, 2-feature pseudo levels): the path that honours `assign` without a fill and takes `fold`. */
int nr3d_lotd_pair_path_ok(const nr3d_lotd_meta_t *meta);
/* pseudo levels of a pair-path meta whose dL/dparam is accumulated straight from (x, dL_dy) in LDS instead of through
 * records (levels with <= 4 buckets; 0 when the pair path does not apply or NR3D_OPT_PAIR_DIRECT is 0).  Informational: which
 * kernel serves which level (bench.py's per-kernel byte model). */
int nr3d_lotd_pair_direct_levels(const nr3d_lotd_meta_t *meta, uint32_t n_points);
/* which pseudo levels (bit q) nr3d_lotd_fwd serves from LDS for a batch of n_points: Dense levels whose whole table fits; 0 when the
 * two-lane forward does not apply.  bench.py prices the forward kernels on the levels each serves. */
uint64_t nr3d_lotd_fwd_lds_levels(const nr3d_lotd_meta_t *meta, uint32_t n_points);
/* size of the `fold` buffer of nr3d_lotd_bwd_dx / nr3d_lotd_bwd_dparam for n_points and max_level; 0 when the folded route does
 * not apply (NR3D_OPT_PAIR_FOLD off, not a pair-path meta, more points than one dL/dparam pass, levels up to max_level not the
 * leading pseudo levels). */
uint64_t nr3d_lotd_pair_fold_bytes(const nr3d_lotd_meta_t *meta, uint32_t n_points, int32_t max_level);

/* lod_bwd, parameter-gradient half (kernel_lod[_hashonly]_backward_grid, lotd_encoding.h:467-711, lotd_hash_only.h:380-470), and
 * (ii) of lod_bwd_bwd_input below, d(dL/dx)/dparam (lotd_encoding.h:764-1041, lotd_hash_only.h:472-574): the one parameter-gradient
 * entry of a single block.
 *   dL_dy, grad_dtype   [N, E] with strides (dldy_sn, dldy_se), float or __half; the feature-major float copy that nr3d_lotd_bwd_dx
 *                       (dL_dy_T) or nr3d_lotd_dLdy_feature_major leaves is passed with strides (1, n_points) and saves the
 *                       transposition here.
 *   dL_ddLdx            NULL: dL/dparam.  float [N, D]: d(dL/dx)/dparam for it (as nr3d_lotd_forest_bwd_dparam).
 *   x                   float [N, D].
 *   params, param_dtype the tables, always passed (the Dense / Hash levels' record routes do not read them).
 *   batch_*, n_batches  as above; n_batches: number of table sets behind `params` when a batch argument is used (the reference
 *                       derives it from params.numel(); 0 = unknown: such a call takes the atomic kernels), 0 or 1 otherwise.
 *   min_level..max_level  the levels computed; the entries of other levels in dL_dparam are not touched.  min_level > 0 has no
 *                       reference counterpart (it only has max_level): a data-parallel caller computes the gradient in level
 *                       buckets and starts the all-reduce of a finished bucket -- a contiguous slice of dL_dparam, levels are stored
 *                       one after another -- while the next bucket is accumulated (bench.py, nr3d_lib_amd/distributed.py).  Per
 *                       level the arithmetic is that of the one-call gradient; how a hot table slice is split over workgroups
 *                       follows the records of the call, so the buckets together equal the one-call result to fp32 rounding of the
 *                       partial sums (each is an fp64 sum), not bitwise.
 *   dL_dparam, out_dtype  float or __half, the numel of params.
 *   assign              0: dL_dparam is ZERO-INIT by the caller and accumulated into.  != 0: dL_dparam arrives UNINITIALISED and is
 *                       fully defined on return: the pair-record path writes instead of read-modify-writing when one first-order
 *                       pass covers every level; in every other case (several passes, a level range, another meta, no or too
 *                       small a workspace, second order, nothing to do: n_points == 0, max_level <= -1, min_level > max_level) the
 *                       library zero-fills (n_batches ? n_batches : 1) * n_params elements first and accumulates.
 *   workspace           optional device scratch of >= nr3d_lotd_dparam_workspace_bytes() bytes: with it (and no 4-D NPlaneMul /
 *                       NPlaneSum level) the gradient is computed atomic-free (binned records + fp64 LDS accumulation); NULL / too
 *                       small / those levels: hardware f32 atomics.
 *   fold                NULL, or (ABI 12, NR3D_OPT_PAIR_FOLD) both gradients of one backward on the pair path in fewer launches:
 *                       nr3d_lotd_bwd_dx (row-major dL_dy) fills `fold` (uninitialised, >= nr3d_lotd_pair_fold_bytes() bytes; a
 *                       size of 0: pass NULL) with what the dL/dparam launches used to make in launches of their own -- the max
 *                       |dL/dy| of the levels up to max_level (the fixed-point scale, bit for bit) and zeroed tickets.  This call
 *                       takes the same n_points, max_level and `fold`, enqueued after it on the same stream, before any other call
 *                       that uses `fold`; results are bit for bit those of the calls with fold == NULL.
 * Half grad_dtype / out_dtype are served where nr3d_lotd_half_params_ok says so, and are an error where the pair-record path does
 * not take the call (no workspace included); a float call falls back to the atomic kernels.  Refused: min_level < 0; dtype codes
 * other than NR3D_F32 / NR3D_F16; second order with min_level > 0, half grad_dtype / out_dtype or fold; half grad_dtype /
 * out_dtype with min_level > 0 or any batch argument; fold with min_level > 0. */
int nr3d_lotd_bwd_dparam(const nr3d_lotd_meta_t *meta, const void *meta_dev, uint32_t n_points,
                         int grad_dtype, const void *dL_dy, int64_t dldy_sn, int64_t dldy_se,
                         const void *dL_ddLdx, const void *x, int param_dtype, const void *params,
                         const int64_t *batch_inds, const int64_t *batch_offsets, uint32_t batch_data_size, uint32_t n_batches,
                         int32_t min_level, int32_t max_level, int out_dtype, int assign, void *dL_dparam,
                         void *workspace, uint64_t workspace_bytes, void *fold, void *stream);

/* lod_bwd_bwd_input (lotd_torch_api.cu:575-729), three independent outputs:
 * (i)  dL_ddLdy[i, e] = sum_d dL_ddLdx[i, d] * dy_dx[i, e, d]      (lotd_encoding.h:1703-1727) */
int nr3d_lotd_bwd_bwd_ddLdy(const nr3d_lotd_meta_t *meta, uint32_t n_points, int x_dtype, int param_dtype,
                            const void *dL_ddLdx, const void *dy_dx, int64_t dydx_sn, int64_t dydx_se,
                            void *dL_ddLdy, int64_t out_sn, int64_t out_se, void *stream);
/* (ii) d(dL/dx)/dparam: nr3d_lotd_bwd_dparam with dL_ddLdx. */
/* (iii) d(dL/dx)/dx (lotd_encoding.h:1157-1298, lotd_hash_only.h:576-695); dL_dx [N, D] fully written.
 * workspace: optional device scratch of nr3d_lotd_bwd_bwd_dx_workspace_bytes(meta, n_points) bytes (0: not served -- Dense /
 * Hash metas only).  With it the pseudo levels of a point are worked on side by side (one lane per (point, pseudo level), the
 * forward's level-major schedule) and summed in level order afterwards; NULL / 0 / too short: one after another in one lane.
 * Same values (the same bits for 2-feature pseudo levels). */
uint64_t nr3d_lotd_bwd_bwd_dx_workspace_bytes(const nr3d_lotd_meta_t *meta, uint32_t n_points);
int nr3d_lotd_bwd_bwd_dx(const nr3d_lotd_meta_t *meta, const void *meta_dev, uint32_t n_points,
                         int x_dtype, int param_dtype, const void *dL_ddLdx,
                         const void *dL_dy, int64_t dldy_sn, int64_t dldy_se, const void *x,
                         const void *params, const int64_t *batch_inds, const int64_t *batch_offsets,
                         uint32_t batch_data_size, int32_t max_level, void *dL_dx, void *workspace,
                         uint64_t workspace_bytes, void *stream);

/* lod_get_grid_index (lotd_torch_api.cu:771-855; kernel lotd_encoding.h:1300-1433):
 * grid_inds int64 [N, n_encoded_dims, 2^D] contiguous, ZERO-INIT.  Dense/Hash levels only. */
int nr3d_lotd_grid_index(const nr3d_lotd_meta_t *meta, const void *meta_dev, uint32_t n_points, int x_dtype,
                         const void *x, const int64_t *batch_inds, const int64_t *batch_offsets,
                         uint32_t batch_data_size, int32_t max_level, int64_t *grid_inds, void *stream);

/* =================================================================================================
 * Forest of blocks -- replaces nr3d_lib.bindings._forest.ForestMeta and the forest overloads of
 * nr3d_lib.bindings._lotd (csrc/forest/forest_cpp_api.h:18-37, csrc/forest/forest.h:25-97,
 * csrc/lotd/src/lotd.cpp:44-60, csrc/lotd/include/lotd/lotd_forest.h).
 * The octree is the breadth-first byte octree of a kaolin SPC: one occupancy byte per non-leaf node (child
 * index = x<<2 | y<<1 | z), exsum = exclusive prefix sum of the bytes' popcounts, node 0 = root; the blocks are
 * the nodes on `level`, block index = node index - level_poffset, block_ks their integer coordinates.
 * All three arrays are DEVICE pointers; the struct itself lives on the host and is passed by value to kernels.
 * ============================================================================================== */
typedef struct nr3d_forest_meta {
	const uint8_t *octree;        /* [n_nodes] */
	const int32_t *exsum;         /* [n_nodes + 1] */
	const int16_t *block_ks;      /* [n_trees, 3] */
	float world_block_size[3];
	float world_origin[3];
	int32_t resolution[3];
	uint32_t n_trees;
	uint32_t level;
	uint32_t level_poffset;
	int32_t continuity_enabled;   /* look corner values up in the neighbouring block across block faces */
} nr3d_forest_meta_t;

/* block index (or -1) of integer block coordinates ks (int16 [n,3]) -- `identify`, forest.h:25-58 /
 * ForestMetaRef::map_block_ind :88-95 (the reference queries through kaolin's unbatched_query on the host side,
 * nr3d_lib/models/spatial/forest.py:244-260). */
int nr3d_forest_identify(const nr3d_forest_meta_t *forest, uint64_t n, const int16_t *ks, int32_t *block_inds,
                         void *stream);

/* lod_fwd(metas=(lod_meta, forest_meta), ...)  (lotd_torch_api.cu:333-361, kernel_lod_forest lotd_forest.h:158-333).
 * x in [0,1]^3 INSIDE the point's block; block_inds int64 [N] (<0: the point is skipped, outputs zero) or NULL with
 * batch_data_size (points per block, blocks in order) or neither (block 0); block_offsets int64 [n_trees] or NULL
 * (block b's parameters start at b * n_params).  f32, D == 3, level types Dense / VectorMatrix / NPlaneMul / CP / Hash
 * (the reference's forest kernels handle no others).  y[i*y_sn + e*y_se]; dy_dx[i*d_sn + e*d_se + d] or NULL
 * (strides in elements, as for nr3d_lotd_fwd; feature-major storage y_sn = 1, y_se = N makes the stores coalesced). */
int nr3d_lotd_forest_fwd(const nr3d_lotd_meta_t *meta, const void *meta_dev, const nr3d_forest_meta_t *forest,
                         uint32_t n_points, const float *x, const void *params, int param_dtype /* NR3D_F32 | NR3D_F16 */,
                         const int64_t *block_inds,
                         const int64_t *block_offsets, uint32_t batch_data_size, int32_t max_level, float *y,
                         int64_t y_sn, int64_t y_se, float *dy_dx, int64_t d_sn, int64_t d_se, void *stream);

/* scratch for the atomic-free forest parameter gradient (per-corner records: a corner may belong to a neighbouring
 * block; Dense / Hash / VecZMatXoY / CP / NPlaneMul / VM levels, lotd_forest.h:415-636); 0 = not applicable (atomics). */
uint64_t nr3d_lotd_forest_dparam_workspace_bytes(const nr3d_lotd_meta_t *meta, uint32_t n_points, uint32_t n_trees);
/* dL/dparam (dL_ddLdx == NULL; kernel_lod_forest_backward_grid :414-542) or d(dL/dx)/dparam
 * (kernel_lod_forest_backward_input_backward_grid :636-773).  dL_dparam [n_trees * n_params] ZERO-INIT by the caller;
 * contributions of corners that lie in a neighbouring block go to that block's parameters.
 * workspace: >= nr3d_lotd_dparam_workspace_bytes(meta, n_points, n_trees) bytes of device scratch, or NULL.  With it,
 * metas whose levels are all Dense / Hash take the atomic-free sort + segmented-sum path of nr3d_lotd_bwd_dparam (the
 * blocks play the role of batch entries; a corner owned by a neighbour is binned into that block's table); otherwise
 * (or when the path does not apply) fp32 hardware atomics. */
int nr3d_lotd_forest_bwd_dparam(const nr3d_lotd_meta_t *meta, const void *meta_dev, const nr3d_forest_meta_t *forest,
                                uint32_t n_points, const float *dL_ddLdx, const float *dL_dy, const float *x,
                                const void *params, int param_dtype, const int64_t *block_inds, const int64_t *block_offsets,
                                uint32_t batch_data_size, int32_t max_level, float *dL_dparam, void *workspace,
                                uint64_t workspace_bytes, void *stream);

/* d(dL/dx)/dx (kernel_lod_forest_backward_input_backward_input :929-1065): Dense / VectorMatrix / Hash levels
 * contribute.  dL_dx [N,3] is overwritten.  (dL/dx and dL/d(dL/dy) are contractions with dy_dx:
 * nr3d_lotd_bwd_dx / nr3d_lotd_bwd_bwd_ddLdy.) */
int nr3d_lotd_forest_bwd_bwd_dx(const nr3d_lotd_meta_t *meta, const void *meta_dev, const nr3d_forest_meta_t *forest,
                                uint32_t n_points, const float *dL_ddLdx, const float *dL_dy, const float *x,
                                const void *params, int param_dtype, const int64_t *block_inds, const int64_t *block_offsets,
                                uint32_t batch_data_size, int32_t max_level, float *dL_dx, void *stream);

/* =================================================================================================
 * Occupancy-grid ray marching -- replaces nr3d_lib.bindings._occ_grid
 *   csrc/occ_grid/include/occ_grid/cpp_api.h:14-66, csrc/occ_grid/src/ray_marching.cu:136-244,
 *   csrc/occ_grid/src/batched_marching.cu:153-287
 * and the ATen chains around it.  Every marcher of this section (static, one call, time-sliced, forest) lives in csrc/occ_grid.hip.
 * Two-phase: *_count writes num_steps[n_rays] AND the exclusive scan packed_info[n_rays,2]
 * (= [cumsum - num, num], int32) plus the grand total into totals[0] (device int32/int64);
 * the caller reads the totals back (the single host sync), allocates outputs, calls *_emit.
 * total_steps / total / totals of the count entry points may be DEVICE memory (then copy it back) or pinned, device-visible HOST
 * memory (hipHostMalloc): the scan's last store lands there and the readback is a stream synchronisation, no copy launch.
 * Optional sample cache (>= nr3d_ray_marching_cache_bytes(n_rays, max_steps) bytes, or NULL): *_count also stores
 * every sample in it and *_emit(sample_cache, cache_max_steps = that max_steps) becomes a parallel compaction
 * instead of a second march (the reference always marches twice, ray_marching.cu:170-240).
 *   grid_binary: uint8/bool [ (B,) Rx, Ry, Rz ], z contiguous.  roi: f32 [6] or [B,6].
 *   batched != 0: batch_inds int32 [n_rays] or NULL (<0 skips), batch_data_size as for LoTD.
 * ============================================================================================== */
enum { NR3D_CONTRACT_AABB = 0, NR3D_CONTRACT_UN_BOUNDED_TANH = 1, NR3D_CONTRACT_UN_BOUNDED_SPHERE = 2 };

/* ---- static grid(s): count | readback | emit ------------------------------------------------------
 * with_hit_rays == 0: packed_info and totals[0] = S, the number of samples; totals is ONE word, ridx_hit / pack_infos are ignored.
 * with_hit_rays != 0: the same AND the per-ray post-processing of occgrid_raymarch.py:87-112 (nonzero on the counts, index, .long())
 * with ONE scan of the counts: the rays with >= 1 sample, ascending, go to ridx_hit int64 [n_rays] / pack_infos int64 [n_rays, 2]
 * (their first n_hit rows are written; both required when n_rays > 0) and totals int64 [2] = {S, n_hit} (the caller reads n_hit back).
 * n_rays == 0 zeroes exactly the words of its mode, one or two.  scan_tmp >= nr3d_scan_tmp_bytes(n_rays).
 * Range of the compacting entry points (with_hit_rays != 0, the one-call and time-sliced marchers below, nr3d_prune_compact_packs):
 * one scan carries the running sample count (36 bits) and the rank among the non-empty packs (28 bits) -- fewer than 2^28 packs /
 * rays per call (checked: nonzero status above that), fewer than 2^36 samples in all (more than a 288 GB device can hold). */
int nr3d_ray_marching_count(uint32_t n_rays, const float *rays_o, const float *rays_d, const float *t_min,
                            const float *t_max, const float *roi, const int32_t grid_res[3],
                            const uint8_t *grid_binary, int contraction_type, float step_size,
                            float max_step_size, float dt_gamma, uint32_t max_steps, int batched,
                            const int32_t *batch_inds, uint32_t batch_data_size,
                            int32_t *packed_info /*[n_rays,2]*/, int64_t *totals /*[1] or [2]*/,
                            void *scan_tmp /* >= nr3d_scan_tmp_bytes(n_rays) bytes */,
                            void *sample_cache /*or NULL*/, uint64_t sample_cache_bytes, int with_hit_rays,
                            int64_t *ridx_hit /*[n_rays]*/, int64_t *pack_infos /*[n_rays,2]*/, void *stream);
/* The samples to their packed rows: t_starts / t_ends f32, ridx int32 (/ bidx / gidx int32).  With the sample cache of the count
 * entry ONE launch, a per-ray copy; without it the second march.  Per-sample post-processing of the same lines, each output optional
 * (NULL): ridx64 = (int64) ridx, deltas = t_ends - t_starts, samples [S, 3] = fma(rays_d[ridx], t_starts, rays_o[ridx])
 * (torch.addcmul).  It rides on the cached copy; behind the second march this entry enqueues it as a launch of its own over n_samples
 * rows (n_samples = S of the readback; read on that route only).  The same values on both routes. */
int nr3d_ray_marching_emit(uint32_t n_rays, const float *rays_o, const float *rays_d, const float *t_min,
                           const float *t_max, const float *roi, const int32_t grid_res[3],
                           const uint8_t *grid_binary, int contraction_type, float step_size,
                           float max_step_size, float dt_gamma, int batched, const int32_t *batch_inds,
                           uint32_t batch_data_size, const int32_t *packed_info, float *t_starts,
                           float *t_ends, int32_t *ridx, int32_t *bidx /*NULL unless batched*/,
                           int32_t *gidx /*or NULL*/, const void *sample_cache /*or NULL*/,
                           uint32_t cache_max_steps, int64_t *ridx64, float *deltas, float *samples, uint64_t n_samples,
                           void *stream);

/* ---- static grid, configs[2] in ONE call (round 6) ------------------------------------------------
 * ray_marching (csrc/occ_grid/src/ray_marching.cu:136-244) + the post-processing of
 * occgrid_raymarch.py:87-112 + alpha = 1 - exp(-sigma * delta) (nerf_utils.py:23-24) + the renderer's composite chain
 * (nr3d_lib/models/fields/nerf/renderer_mixin.py:298-311), enqueued back to back with NO device->host wait inside:
 *   count (+ sample cache) -> scan (+ hit rays, totals) -> cached emit (+ ridx64 / deltas / samples) -> composite over ALL rays.
 * Every per-sample buffer (t_starts, t_ends, ridx, gidx?, ridx64?, deltas, samples?, alphas, vw) has `rows` >= n_rays * max_steps
 * rows (the bound; checked) and its first S rows are written -- the same values as nr3d_ray_marching_count (with_hit_rays) +
 * nr3d_ray_marching_emit + nr3d_tau_to_alpha_fwd + nr3d_pack_composite_fwd, vw / mask / depth / rgb_out bit-identical to
 * them.  sigma [sigma_rows] / rgb [sigma_rows, 3] (rgb optional): the caller's per-sample density / colour; rows beyond sigma_rows
 * read as density 0 (the caller compares S with sigma_rows after its readback).  mask / depth [n_rays], rgb_out [n_rays, 3] are
 * FULLY written (rays without samples: zeros -- no fill).  totals (device-visible, normally pinned host memory) = {S, n_hit}: read it
 * after a stream synchronisation, AFTER this call returned (and after nr3d_march_composite_bwd was enqueued, if wanted).
 * Needs the sample cache (nr3d_ray_marching_cache_bytes); single grid only (batched / forest marches keep the two-phase calls). */
int nr3d_march_composite_fwd(uint32_t n_rays, const float *rays_o, const float *rays_d, const float *t_min, const float *t_max,
                             const float *roi, const int32_t grid_res[3], const uint8_t *grid_binary, int type, float step_size,
                             float max_step_size, float dt_gamma, uint32_t max_steps, int32_t *packed_info, int64_t *ridx_hit,
                             int64_t *pack_infos, int64_t *totals, void *scan_tmp, void *sample_cache, uint64_t sample_cache_bytes,
                             uint64_t rows, float *t_starts, float *t_ends, int32_t *ridx, int32_t *gidx, int64_t *ridx64,
                             float *deltas, float *samples, const float *sigma, uint64_t sigma_rows, const float *rgb,
                             float early_stop_eps, float alpha_thre, int normalize_depth, float *alphas, float *vw, float *mask,
                             float *depth, float *rgb_out, void *stream);
/* its backward (= nr3d_pack_composite_bwd over all rays of packed_info, no ray_index, no g_vw; the same values): g_mask / g_depth
 * [n_rays], g_rgb [n_rays, 3] (each may be NULL = zero) -> grad_alphas [S rows written], grad_t / grad_rgb optional; grad_sigma
 * (optional, needs sigma and deltas) = grad_alphas * exp(-sigma * delta) * delta as nr3d_tau_to_alpha_bwd. */
int nr3d_march_composite_bwd(uint32_t n_rays, const int32_t *packed_info, const float *alphas, const float *vw, const float *t,
                             const float *rgb, float early_stop_eps, float alpha_thre, int normalize_depth, const float *mask,
                             const float *depth, const float *g_mask, const float *g_depth, const float *g_rgb, float *grad_alphas,
                             float *grad_t, float *grad_rgb, const float *sigma, const float *deltas, uint64_t sigma_rows,
                             float *grad_sigma, void *stream);

/* ---- dynamic scenes: the march through TIME-SLICED occupancy, every ray with a timestamp ----------
 * No single reference kernel: replaces the
 * chain of models/accelerations/occgrid_accel/dynamic.py:117-151, :328-364 and batched_dynamic.py:69-110
 * (torch_consecutive_nearest1d -> `occ_dynamic | occ_static.expand_as(...)` -> batched march -> ts_keyframes[bidx] -> div / sub).
 *   grid_dynamic uint8 [n_slices, Rx, Ry, Rz], n_slices = (batch_inds ? n_batches : 1) * T; grid_static uint8 [Rx, Ry, Rz] or NULL
 *   (a cell is occupied when either byte is nonzero); roi [6]; AABB grids only.  ts_keyframes [T] ascending, rays_ts [n_rays].
 *   Frame of a ray = torch_consecutive_nearest1d (nr3d_lib/utils.py:675-699), the same float32 operations: i = first index with
 *   key[i] >= t (NaN: T), clamped to [1, T-1]; frame i-1 if |key[i-1] - t| < |key[i] - t| else i; T == 1: frame 0.
 *   slice = (batch_inds ? batch_inds[i] : 0) * T + frame -> rays_slice int32 [n_rays]; a ray whose batch index is negative or
 *   >= n_batches gets slice -1, count 0 and is never probed.  n_slices * Rx*Ry*Rz >= 2^31 is refused (gidx is int32).
 * _count: packed_info / ridx_hit / pack_infos / totals = {S, n_hit} / scan_tmp as nr3d_ray_marching_count with with_hit_rays != 0;
 * the sample cache (nr3d_ray_marching_cache_bytes) is required.  _emit (after the caller read totals = {S, n_hit}): per sample t_starts, t_ends,
 * ridx int64, bidx int64 (= batch_inds of the ray; NULL without batch_inds), ts = ts_keyframes[frame], gidx int32 (cell + slice *
 * Rx*Ry*Rz; optional), deltas = t_ends - t_starts, samples [S, 3] = rays_o + (rays_d * t_starts) with the product rounded on its own --
 * torch.addcmul's float32 result on the chain's route (self + value * (t1 * t2)), so the two routes agree bit for bit. */
int nr3d_dynamic_ray_marching_count(uint32_t n_rays, const float *rays_o, const float *rays_d, const float *t_min,
                                    const float *t_max, const float *roi, const int32_t grid_res[3],
                                    const uint8_t *grid_dynamic, const uint8_t *grid_static, const float *ts_keyframes,
                                    uint32_t T, const float *rays_ts, const int32_t *batch_inds, uint32_t n_batches,
                                    float step_size, float max_step_size, float dt_gamma, uint32_t max_steps,
                                    int32_t *packed_info, int32_t *rays_slice, int64_t *ridx_hit, int64_t *pack_infos,
                                    int64_t *totals, void *scan_tmp, void *sample_cache, uint64_t sample_cache_bytes,
                                    void *stream);
int nr3d_dynamic_ray_marching_emit(uint32_t n_rays, const float *rays_o, const float *rays_d, const float *ts_keyframes,
                                   uint32_t T, const int32_t *batch_inds, const int32_t *packed_info,
                                   const int32_t *rays_slice, const void *sample_cache, uint32_t cache_max_steps,
                                   float *t_starts, float *t_ends, int64_t *ridx, int64_t *bidx, float *ts, int32_t *gidx,
                                   float *deltas, float *samples, void *stream);
/* the frame lookup alone: fidx int64 [n] = nearest keyframe of ts [n] (as above) */
int nr3d_nearest_keyframe(uint64_t n, const float *ts_keyframes, uint32_t T, const float *ts, int64_t *fidx, void *stream);

/* ---- forest of block grids ------------------------------------------------------------------------
 * forest_ray_marching (csrc/occ_grid/src/forest_marching.cu:16-303): marching through the occupancy grids of the
 * blocks a ray crosses.  The block segments of every ray (seg_block_inds int32 [S], seg_entries / seg_exits f32 [S],
 * packed per ray by seg_pack_infos int32 [n_rays,2]) come from the caller's octree ray trace.
 * grid_binary uint8/bool [n_trees, Rx, Ry, Rz].  Same two-phase contract as nr3d_ray_marching_count (with_hit_rays == 0) / _emit
 * (no sample cache: always the second march). */
int nr3d_forest_ray_marching_count(const nr3d_forest_meta_t *forest, uint32_t n_rays, const float *rays_o,
                                   const float *rays_d, const float *t_min, const float *t_max,
                                   const int32_t *seg_block_inds, const float *seg_entries, const float *seg_exits,
                                   const int32_t *seg_pack_infos, const int32_t grid_res[3], const uint8_t *grid_binary,
                                   float step_size, float max_step_size, float dt_gamma, uint32_t max_steps,
                                   int32_t *packed_info /*[n_rays,2]*/, int64_t *total_steps /*[1]*/, void *scan_tmp,
                                   void *stream);
int nr3d_forest_ray_marching_emit(const nr3d_forest_meta_t *forest, uint32_t n_rays, const float *rays_o,
                                  const float *rays_d, const float *t_min, const float *t_max,
                                  const int32_t *seg_block_inds, const float *seg_entries, const float *seg_exits,
                                  const int32_t *seg_pack_infos, const int32_t grid_res[3], const uint8_t *grid_binary,
                                  float step_size, float max_step_size, float dt_gamma, const int32_t *packed_info,
                                  float *t_starts, float *t_ends, int32_t *ridx, int32_t *blidx, int32_t *gidx /*or NULL*/,
                                  void *stream);

/* ---- sizes and the readback ------------------------------------------------------------------------
 * Bytes of the marchers' sample cache ([n_rays][max_steps] x {t_start, t_end, cell}). */
uint64_t nr3d_ray_marching_cache_bytes(uint32_t n_rays, uint32_t max_steps);
/* Scratch bytes needed by the device-wide scans used in two-phase ops (any n). */
uint64_t nr3d_scan_tmp_bytes(uint64_t n);
/* Host-side wait for words a kernel writes into device-visible HOST memory (pinned; the `totals` of the two-phase and one-call ops):
 * spins until none of words[0..n) equals `sentinel` (the caller stores the sentinel before the launch; the kernels store the totals
 * with system scope) or `timeout_us` passed.  Returns 0 when the words arrived, 1 on timeout (NOT an error: the caller falls back to a
 * stream synchronisation).  Why: a stream synchronisation returns when EVERYTHING enqueued has drained and costs ~20 us of wake-up
 * latency; the totals are written by the SECOND of the one-call path's launches, and reading them early lets the host build its views
 * while the composite kernels still run.  Holds no lock, touches no HIP API. */
int nr3d_wait_host_words(const int64_t *words, int n, int64_t sentinel, uint32_t timeout_us);

/* Occupancy-value grid maintenance -- replaces torch_scatter.scatter_max in update_occ_val_grid[_idx]_ /
 * update_batched_occ_val_grid[_idx]_ (nr3d_lib/models/accelerations/occgrid/utils.py:80-125):
 *   grid[v] <- max(ema_decay * grid[v], max_{samples in v} occ_val)  for touched voxels, unchanged otherwise.
 * scatter_max: vmax [n_batches * Rx*Ry*Rz] f32 scratch := -inf, then the per-voxel maximum of occ_val.  Voxel of
 *   sample i: gidx[i] (int64 [n,3]) or, when gidx == NULL, ((pts[i]/2 + 0.5) * res).long().clamp(0, res-1);
 *   batch of sample i: bidx[i] (int64) or i / per_batch (per_batch == 0: single grid).
 * apply_max: applies the decayed maximum in place.  A sharded caller all-reduces(MAX) vmax between the two. */
int nr3d_occ_scatter_max(uint64_t n, const int64_t *gidx, const float *pts, const int64_t *bidx, uint64_t per_batch,
                         const float *occ_val, const int32_t grid_res[3], uint32_t n_batches, float *vmax, void *stream);
int nr3d_occ_apply_max(uint64_t n_voxels, float ema_decay, const float *vmax, float *occ_val_grid, void *stream);

/* =================================================================================================
 * Fused fully-connected decoder -- the MLP right after the encoder: nr3d_lib/models/blocks/mlp.py:27-127 (`MLP` /
 * `FCBlock`: D hidden DenseLayers + an output layer, nr3d_lib/models/layers.py:228-300), in the reference a chain of
 * GEMM + elementwise launches (or tiny-cuda-nn's fused fp16 network behind nr3d_lib/models/tcnn_adapter.py:74-237).
 * fp32 in / fp32 accumulate; the whole network in one kernel, activations in registers.  Forward: on the bf16 MFMA with every value
 * split into three bf16 pieces and the six significant piece products (fp32-grade; NR3D_OPT_MLP_X3, ABI 5) or on the f32 MFMA; backward:
 * f32 MFMA.  The packed buffer holds [f32 layers | the layers' bf16 pieces | transposed f32 layers (with_backward)]: opaque to the caller.
 *   dims[0] = in_features, dims[1..n_layers-1] = hidden widths, dims[n_layers] = out_features; every width 1..128;
 *   weights[l]: f32 [dims[l+1], dims[l]] row-major (torch nn.Linear layout), biases[l]: f32 [dims[l+1]] or NULL.
 * nr3d_mlp_packed_floats: size of the packed-weights buffer, or 0 when the fused kernels do not apply (a single
 *   layer, a width > 128, packed weights beyond the LDS budget) -- the caller then keeps its unfused path.
 * nr3d_mlp_pack: weights/biases (HOST arrays of n_layers DEVICE pointers) -> packed, in MFMA operand order; call it
 *   whenever the parameters changed (once per optimiser step).
 * nr3d_mlp_forward: y[i*y_stride + o] for x[i*x_stride + f*x_feature_stride], x either row-major (x_feature_stride == 1;
 *   rows need not be padded or aligned, 16-byte aligned rows take vector loads) or feature-major (x_stride == 1: the
 *   [E, N] storage the LoTD kernels write, consumed without a transposing copy -- a half-wave then reads 128 contiguous
 *   bytes of one feature).  nr3d_mlp_backward takes x the same way and stores dL_dx in either layout
 *   (gx_stride / gx_feature_stride; feature-major dL_dx is what nr3d_lotd_bwd_dparam reads without its transposition
 *   pass).
 * ============================================================================================== */
#define NR3D_MLP_MAX_LAYERS 8
/* NR3D_MLP_ACT_SOFTPLUS (ABI 19): torch.nn.Softplus(beta = softplus_beta, threshold = 20) -- h = z where beta z > 20, else
 * log1p(exp(beta z)) / beta, evaluated on the fp32 accumulator -- the activation of the reference's SDF decoders
 * (nr3d_lib/models/fields/sdf/mlp_sdf.py:30: {'type': 'softplus', 'beta': 100.}).  A HIDDEN activation only, on the forward and the
 * first backward of both precisions: as output_activation, or with a softplus_beta that is not finite or not > 0, every size query
 * below returns 0 (the caller keeps its unfused path).  A valid softplus network has the sizes of the same dims with ReLU.
 * nr3d_mlp_backward_backward does not take it (nr3d_mlp_backward_backward_ok returns 0: the network is not piecewise linear); its
 * double backward is nr3d_mlp_softplus_backward_backward (ABI 21), which also produces dL/db and dL/dx.
 *
 * NR3D_MLP_ACT_SIGMOID (ABI 22): y = 1 / (1 + exp(-z)) on the fp32 accumulator z of the OUTPUT layer -- in the half kernels before the
 * result is rounded to half -- the output activation of the reference's radiance decoders (nr3d_lib/models/fields/nerf/mlp_nerf.py:196,
 * lotd_nerf.py:219-224: 32 -> 64 -> 64 -> 3, ReLU hidden layers).  An OUTPUT activation only, with any hidden activation the kernels
 * take (none, ReLU, softplus), on the forward and the first backward of both precisions; the backward recomputes z and scales dL/dy by
 * sigmoid'(z), no y is kept.  A sigmoid network has the sizes of the same dims with a ReLU output.  Neither double backward takes it
 * (both _ok queries return 0, both entries fail with a message): the caller differentiates its unfused path.
 *
 * Any other combination -- sigmoid as hidden_activation, softplus as output_activation, a code outside this enum in either field -- is
 * refused: every size query returns 0 and every entry fails with a message (ABI 22; before, an unknown code ran as the identity). */
enum { NR3D_MLP_ACT_NONE = 0, NR3D_MLP_ACT_RELU = 1, NR3D_MLP_ACT_SOFTPLUS = 2, NR3D_MLP_ACT_SIGMOID = 3 };

typedef struct nr3d_mlp_desc {
	uint32_t n_layers;                          /* linear layers: hidden layers + 1 */
	uint32_t dims[NR3D_MLP_MAX_LAYERS + 1];
	uint32_t hidden_activation;                 /* after every hidden layer: NR3D_MLP_ACT_NONE, _RELU or _SOFTPLUS */
	uint32_t output_activation;                 /* NR3D_MLP_ACT_NONE, _RELU or _SIGMOID (ABI 22: y = 1 / (1 + exp(-z)) on the output layer's
	                                             * fp32 accumulator; half kernels: before the rounding to half) */
	float softplus_beta;                        /* read only when hidden_activation == NR3D_MLP_ACT_SOFTPLUS (ABI 19; at the end: a
	                                             * zero-initialised desc with ReLU / no activations means what it meant before) */
} nr3d_mlp_desc_t;

uint64_t nr3d_mlp_packed_floats(const nr3d_mlp_desc_t *desc);
/* extra floats of the packed buffer that nr3d_mlp_backward needs (a 4-float header: the backward reads the forward layers), or 0
 * when the fused backward does not apply (hidden width > 64, more than 2 hidden layers wider than 32 / 3 narrower ones, input or output wider
 * than the hidden layers): the caller then differentiates its unfused path. */
uint64_t nr3d_mlp_backward_packed_floats(const nr3d_mlp_desc_t *desc);
/* packed: nr3d_mlp_packed_floats (+ nr3d_mlp_backward_packed_floats when with_backward != 0) floats */
int nr3d_mlp_pack(const nr3d_mlp_desc_t *desc, const float *const *weights, const float *const *biases, float *packed,
                  int with_backward, void *stream);
/* dL/dx (or NULL), dL/dW_l [dims[l+1], dims[l]] and dL/db_l (dL_db or entries may be NULL) from x and dL/dy; the forward
 * is recomputed in registers, nothing but x has to be kept from the forward pass.  Parameter gradients are ADDED to
 * dL_dW / dL_db (fp32 atomics, one per element and workgroup): zero them for plain gradients. */
int nr3d_mlp_backward(const nr3d_mlp_desc_t *desc, uint64_t n, const float *x, int64_t x_stride, int64_t x_feature_stride,
                      const float *dL_dy, int64_t gy_stride, const float *packed, float *dL_dx, int64_t gx_stride,
                      int64_t gx_feature_stride, float *const *dL_dW, float *const *dL_db, void *stream);
int nr3d_mlp_forward(const nr3d_mlp_desc_t *desc, uint64_t n, const float *x, int64_t x_stride, int64_t x_feature_stride,
                     const float *packed, float *y, int64_t y_stride, void *stream);
/* Double backward (ABI 10) -- the create_graph route of an SDF decoder's nablas = dL/dx and the eikonal loss on them (the reference
 * differentiates its GEMM chain twice, or points users at a tiny-cuda-nn fork with a double-backward fused MLP).  Given u = dL_dy
 * (rows, gy_stride 0 allowed: an expanded ones) and v = ddL_dx = dL/d(dL/dx) (layouts as x: row-major or feature-major), with r_l
 * the first backward's dL/d(pre-activation of layer l) and t_l = m_l W_l t_{l-1} (t_{-1} = v, m_l the ReLU masks) the tangent of v:
 *   dL_dW[l] += sum over samples of r_l t_{l-1}^T (fp32 atomics as nr3d_mlp_backward: zero them first);
 *   dL_ddLdy [n, out] rows (ggy_stride; NULL: not wanted) = t_L, fully written;
 *   dL/db_l and dL/dx are zero (the network is piecewise linear) and are not produced.
 * packed comes from nr3d_mlp_pack(..., with_backward = 1); the forward is recomputed with nr3d_mlp_backward's route under the same
 * options (NR3D_OPT_MLP_X3), so the masks are bit for bit the ones its dL/dx used.  nr3d_mlp_backward_backward_ok: 1 when the
 * fused double backward applies (the shapes of nr3d_mlp_backward with ReLU / no hidden activation), else 0: the caller differentiates
 * its unfused path.  Softplus hidden layers are outside it (the network is not piecewise linear: dL/db_l and dL/dx are not zero), and
 * so is a sigmoid output (ABI 22); nr3d_mlp_backward_backward then fails with a message. */
int nr3d_mlp_backward_backward_ok(const nr3d_mlp_desc_t *desc);
int nr3d_mlp_backward_backward(const nr3d_mlp_desc_t *desc, uint64_t n, const float *x, int64_t x_stride, int64_t x_feature_stride,
                               const float *dL_dy, int64_t gy_stride, const float *ddL_dx, int64_t v_stride, int64_t v_feature_stride,
                               const float *packed, float *dL_ddLdy, int64_t ggy_stride, float *const *dL_dW, void *stream);
/* Double backward with softplus hidden layers (ABI 21; the eikonal term of the reference's SDF decoders).  sigma'' = beta s e is not
 * zero (s_l = sigmoid(beta z_l), e_l = 1 - s_l; above the threshold s = 1 and e = 0 exactly, as torch), so with u = dL_dy, v = ddL_dx,
 * r_l / g_l the first backward's chain (r_L = m_L u, g_l = W_{l+1}^T r_{l+1}, r_l = s_l g_l) and t_l = s_l W_l t_{l-1} (t_0 = v):
 *   q_l = beta e_l g_l t_l,   p_NH = q_NH,   p_l = q_l + s_l W_{l+1}^T p_{l+1}                 (hidden layers)
 *   dL_dW[l] += sum over samples of r_l t_{l-1}^T + p_l h_{l-1}^T                               (output layer: the first term only)
 *   dL_db[l] += sum over samples of p_l     (hidden layers; dL_db or entries may be NULL; the output layer's entry is not touched)
 *   dL_dx = W_1^T p_1, fully written, row- or feature-major as nr3d_mlp_backward's (NULL: not wanted)
 *   dL_ddLdy [n, out] rows = m_L W_L t_NH, fully written (NULL: not wanted).
 * x, ddL_dx, dL_dy (gy_stride 0 allowed), packed and the fp32 atomics on dL_dW / dL_db as nr3d_mlp_backward_backward; n == 0 returns 0.
 * nr3d_mlp_softplus_backward_backward_ok: 1 exactly for softplus hidden layers (valid beta, output none or ReLU, not sigmoid) on a shape
 * nr3d_mlp_backward takes and whose launch plan (per-wave LDS tiles about twice those of nr3d_mlp_backward_backward) fits at least one
 * wave; a ReLU / linear desc gives 0 and nr3d_mlp_softplus_backward_backward then fails with a message. */
int nr3d_mlp_softplus_backward_backward_ok(const nr3d_mlp_desc_t *desc);
int nr3d_mlp_softplus_backward_backward(const nr3d_mlp_desc_t *desc, uint64_t n, const float *x, int64_t x_stride, int64_t x_feature_stride,
                                        const float *dL_dy, int64_t gy_stride, const float *ddL_dx, int64_t v_stride,
                                        int64_t v_feature_stride, const float *packed, float *dL_ddLdy, int64_t ggy_stride, float *dL_dx,
                                        int64_t gx_stride, int64_t gx_feature_stride, float *const *dL_dW, float *const *dL_db, void *stream);

/* The same decoder in HALF precision on the f16 MFMA (csrc/mlp_half.hip) -- the contract of the reference's fast decoder,
 * tiny-cuda-nn's FullyFusedMLP behind nr3d_lib/models/tcnn_adapter.py:37-51,74-146 (`use_tcnn_backend`,
 * nr3d_lib/models/blocks/__init__.py:3-15): half weights / biases / inputs / outputs, activations rounded to half between
 * the layers; the dot products of a layer are accumulated in fp32 (tcnn accumulates in half).  x, y, dL_dy, dL_dx: __half,
 * same layout rules as the fp32 entry points (strides in elements; row-major rows 8-byte aligned with widths that are multiples
 * of 4 take the vector / prefetched path).  weights[l] / biases[l]: __half, torch nn.Linear layout.  Sizes are BYTES here.
 * nr3d_mlp_half_backward: dL_dW / dL_db are FP32 buffers the workgroups add their partial sums to (zero them first) -- the
 * caller rounds them to the parameters' dtype; the fused backward applies to the same shapes as nr3d_mlp_backward. */
uint64_t nr3d_mlp_half_packed_bytes(const nr3d_mlp_desc_t *desc);
uint64_t nr3d_mlp_half_backward_packed_bytes(const nr3d_mlp_desc_t *desc);
int nr3d_mlp_half_pack(const nr3d_mlp_desc_t *desc, const void *const *weights, const void *const *biases, void *packed,
                       int with_backward, void *stream);
int nr3d_mlp_half_forward(const nr3d_mlp_desc_t *desc, uint64_t n, const void *x, int64_t x_stride, int64_t x_feature_stride,
                          const void *packed, void *y, int64_t y_stride, void *stream);
int nr3d_mlp_half_backward(const nr3d_mlp_desc_t *desc, uint64_t n, const void *x, int64_t x_stride, int64_t x_feature_stride,
                           const void *dL_dy, int64_t gy_stride, const void *packed, void *dL_dx, int64_t gx_stride,
                           int64_t gx_feature_stride, float *const *dL_dW, float *const *dL_db, void *stream);

/* The weight normalisation of the reference's LipshitzMLP (nr3d_lib/models/blocks/mlp.py:168-249, `normalization`) and its gradient,
 * ONE launch each for all layers of a network (csrc/mlp_lipschitz.hip; additions, the ABI number stays).  Per layer l and row r:
 *   sp = softplus(c[l]) (torch's: beta 1, threshold 20),  a = sum_j |W[r, j]|,  den = max(a, sp) (a NaN propagates, as clamp_min),
 *   normalized[l][r, j] = W[r, j] * (sp / den), rounded once to the weight type; where a < sp that is W[r, j] bit for bit.
 * The decoder entries above then take `normalized` in place of the weights.  Backward, from grads[l] = dL/d normalized[l] (fp32):
 *   S = sum_j grads[l][r, j] W[r, j],  pass = a >= sp (a tie sends the gradient through a),
 *   dL_dW[l][r, j] = grads[l][r, j] sp / den - (pass ? sign(W[r, j]) S (sp / den) / den : 0)      (sign(0) = 0),
 *   dL_dc[l] = softplus'(c[l]) sum_r S_r / den_r -- both fp32 and WRITTEN (no zero fill, no atomics: a fixed summation order, the same
 *   bytes run after run).  Inf, NaN, all-zero rows and an sp that underflows to 0 give what IEEE arithmetic gives, as in the torch chain.
 * rows[l] x cols[l] (HOST arrays, each 1..4096: not restricted to the fused decoder's widths) is the shape of weights[l], row-major and
 * contiguous; weights / normalized / grads / dL_dW: HOST arrays of n_layers DEVICE pointers, as nr3d_mlp_pack takes them (outputs must
 * not alias inputs); weights_half != 0: weights and normalized are __half, else float; c: n_layers floats on the device.
 * n_layers 1..NR3D_MLP_MAX_LAYERS + 1; a zero or too large dimension or a NULL pointer fails with a message. */
int nr3d_mlp_lipschitz_normalize(uint32_t n_layers, const uint32_t *rows, const uint32_t *cols, const void *const *weights,
                                 int weights_half, const float *c, void *const *normalized, void *stream);
int nr3d_mlp_lipschitz_normalize_backward(uint32_t n_layers, const uint32_t *rows, const uint32_t *cols, const void *const *weights,
                                          int weights_half, const float *c, const float *const *grads, float *const *dL_dW,
                                          float *dL_dc, void *stream);

/* =================================================================================================
 * pack_ops -- replaces nr3d_lib.bindings._pack_ops  (csrc/pack_ops/pack_ops.h:11-65,
 * csrc/pack_ops/pack_ops.cpp:21-58, kernels csrc/pack_ops/pack_ops_cuda.cu)
 * pack_infos: int64 [P,2] = (begin, length), contiguous.  feats: [S] or [S, feat_dim] contiguous.
 * ============================================================================================== */

/* n_per_pack (int64 [P]) -> pack_infos [P,2] = (exclusive cumsum, n) and total[0]; the host-side
 * `cumsum` + `stack` of every two-phase pack op (e.g. pack_ops_cuda.cu:584-586). */
int nr3d_pack_infos_from_n(uint32_t P, const int64_t *n_per_pack, int64_t *pack_infos, int64_t *total,
                           void *scan_tmp, void *stream);

/* interleave_arange / interleave_linstep (:47-218).  starts/step_sizes may be NULL (then scalars
 * start_s/step_s are used; passed as double and converted to dtype).  nidx may be NULL. */
int nr3d_interleave_linstep(uint32_t P, int dtype, const int64_t *pack_infos, const void *starts,
                            const void *step_sizes, double start_s, double step_s, void *out,
                            int64_t *nidx, void *stream);
/* the step counts of interleave_arange (graphics/pack_ops/pack_ops.py: stop.subtract(start).div(step_size).ceil().long(), four ATen
 * launches) in one: num_steps[i] = ceil((stops[i] - starts[i]) / step) as int64, the quotient in float32 for int32 / int64 / float32
 * tensors (ATen's true division) and in float64 for float64.  step_sizes [P] of the tensors' dtype, or NULL: the scalar step_s. */
int nr3d_arange_num_steps(uint32_t P, int dtype, const void *starts, const void *stops, const void *step_sizes, double step_s,
                          int64_t *num_steps, void *stream);

/* interleave_sample_step_wrt_depth_clamped (:480-604), round 1 then round 2. */
int nr3d_sample_step_count(uint32_t P, const float *nears, const float *fars, uint32_t max_steps,
                           float dt_gamma, float min_step, float max_step, int64_t *n_per_pack, void *stream);
int nr3d_sample_step_emit(uint32_t P, const float *nears, const int64_t *pack_infos, float dt_gamma,
                          float min_step, float max_step, float *t_samples, float *deltas, int64_t *nidx,
                          void *stream);
/* interleave_sample_step_wrt_depth_in_packed_segments (:606-795): emit == 0 -> n_per_pack. */
int nr3d_sample_step_segments(uint32_t P, const float *nears, const float *fars, const float *entries,
                              const float *exits, const int64_t *seg_pack_infos, uint32_t max_steps,
                              float dt_gamma, float min_step, float max_step, int emit, int64_t *n_per_pack,
                              const int64_t *pack_infos, float *t_samples, float *deltas, int64_t *nidx,
                              int64_t *sidx, void *stream);

/* packed_sum (:798-861).  out [P, feat_dim], fully written (empty packs -> 0). */
int nr3d_packed_sum(uint32_t P, uint64_t S, uint32_t feat_dim, int dtype, const void *feats,
                    const int64_t *pack_infos, void *out, void *stream);
/* Rows of `out` outside every pack (packed_scan / packed_diff / packed_binary; the reference allocates at::zeros):
 *   ordered_packs == 0: the kernel writes the rows of the packs only -- pass a zeroed `out`;
 *   ordered_packs != 0: the caller states pack_infos[p+1].begin >= pack_infos[p].begin + pack_infos[p].len for every p
 *   (what every producer of pack_infos emits: a marcher, an interleave_* op, get_pack_infos_from_n); the kernel then
 *   zeroes the rows in front of the first pack, between packs and behind the last pack (up to S) itself, so `out`
 *   may be uninitialised and no fill launch is needed in front of a launch-bound op. */
/* packed_cumsum / packed_cumprod (:864-1095).  reference first-element semantics. */
int nr3d_packed_scan(uint32_t P, uint64_t S, uint32_t feat_dim, int dtype, const void *feats,
                     const int64_t *pack_infos, int is_prod, int exclusive, int reverse, int ordered_packs,
                     void *out, void *stream);
/* packed_diff / packed_backward_diff (:1098-1333).  edge_a = appends|prepends, edge_fill = last|first fill
 * (at most one non-NULL).  backward != 0 selects packed_backward_diff. */
int nr3d_packed_diff(uint32_t P, uint64_t S, uint32_t feat_dim, int dtype, const void *feats,
                     const int64_t *pack_infos, const void *edge_a, const void *edge_fill, int backward,
                     int ordered_packs, void *out, void *stream);
/* packed_{add,sub,mul,div,gt,geq,lt,leq,eq,neq} (:1960-2480).  op = PackBinaryOpType value
 * (pack_ops.h:25-37: Add 0, Subtract 1, Multiply 2, Division 3, Matmul 4, Gt 5 ... Neq 10).
 * Comparisons write uint8 (bool).  Matmul: other [P, out_dim, feat_dim], out [S, out_dim]. */
int nr3d_packed_binary(uint32_t P, uint64_t S, uint32_t feat_dim, uint32_t out_dim, int dtype,
                       const void *feats, const void *other, const int64_t *pack_infos, int op,
                       int ordered_packs, void *out, void *stream);
/* packed_searchsorted[_packed_vals] (:1336-1503).  val_pack_infos NULL -> vals is [P, num_to_search]. */
int nr3d_packed_searchsorted(uint32_t P, int dtype, const void *bins, const void *vals,
                             const int64_t *pack_infos, uint32_t num_to_search,
                             const int64_t *val_pack_infos, int64_t *pidx, void *stream);
/* try_merge_two_packs_sorted_aligned (:1505-1631).  The rows of the packs are fully written (ABI 5: the kernel zeroes its own
 * counting rows); rows of pidx_a / pidx_b outside every pack keep the caller's fill -- 0 as the reference's aligned op, -1 as its
 * merge_two_packs_sorted. */
int nr3d_try_merge_two_packs_sorted_aligned(uint32_t P, int dtype, const void *vals_a,
                                            const int64_t *pack_infos_a, const void *vals_b,
                                            const int64_t *pack_infos_b, const int64_t *pack_infos_merged,
                                            int b_sorted, int64_t *pidx_a, int64_t *pidx_b, void *stream);
/* merge_two_packs_sorted (graphics/pack_ops/pack_ops.py:611-640: the torch.unique / nonzero / index chain in front of the aligned
 * merge): the UNION of two sorted, unique pack-id lists as ALIGNED descriptors.  Union pack k is (a's pack | an empty one, b's pack |
 * an empty one): u [<= Pa + Pb] ids, pack_infos_a_u / pack_infos_b_u [<= Pa + Pb, 2], n_u [<= Pa + Pb] merged lengths; the first
 * total_u[0] = Pa + (packs of b that a does not have) rows are written; total_u may be pinned host memory, like the other totals
 * (n_only [1] is device scratch).
 * Then: nr3d_pack_infos_from_n(n_u) and nr3d_try_merge_two_packs_sorted_aligned on the aligned descriptors.
 * Scratch: only_b [Pb], ob [Pb, 2] (int64), scan_tmp >= nr3d_scan_tmp_bytes(Pb). */
int nr3d_merge_pack_union(uint32_t Pa, const int64_t *nidx_a, const int64_t *pack_infos_a, uint32_t Pb, const int64_t *nidx_b,
                          const int64_t *pack_infos_b, int64_t *only_b, int64_t *ob, void *scan_tmp, int64_t *n_only,
                          int64_t *u, int64_t *pack_infos_a_u, int64_t *pack_infos_b_u, int64_t *n_u, int64_t *total_u, void *stream);
/* packed_invert_cdf (:1633-1733). */
int nr3d_packed_invert_cdf(uint32_t P, const float *bins, const float *cdfs, const int64_t *pack_infos,
                           const float *u_vals, uint32_t num_to_sample, float *samples, int64_t *bin_idx,
                           void *stream);
/* packed_sort_qsort (:2634-2763): sorts vals IN PLACE per pack; ids (int64 arange, or NULL) permuted. */
int nr3d_packed_sort(uint32_t P, uint64_t S, int dtype, void *vals, int64_t *ids, const int64_t *pack_infos,
                     void *stream);
/* packed_alpha_to_vw_forward (:1735-1793, :1850-1907).  Any of weights / num_steps / selector may be
 * NULL; weights and selector are fully written (skipped samples -> 0). */
int nr3d_alpha_to_vw_forward(uint32_t P, uint64_t S, const float *alphas, const int64_t *pack_infos,
                             float early_stop_eps, float alpha_thre, float *weights, int64_t *num_steps,
                             uint8_t *selector, void *stream);
/* packed_alpha_to_vw_backward (:1795-1848, :1910-1958).  grad_alphas fully written. */
int nr3d_alpha_to_vw_backward(uint32_t P, uint64_t S, const float *alphas, const float *weights,
                              const float *grad_weights, const int64_t *pack_infos, float early_stop_eps,
                              float alpha_thre, float *grad_alphas, void *stream);
/* Fused alpha composite of a packed volume buffer.  No single reference kernel: replaces the renderer's op chain
 * nr3d_lib/models/fields/nerf/renderer_mixin.py:298-311 = packed_alpha_to_vw (pack_ops_cuda.cu:1735-1793) ->
 * packed_sum (:798-861) -> packed_div (:1960-2062) -> packed_sum(. * t) -> packed_sum(. * rgb), and its autograd
 * (pack_ops.py:97-116, :261-283, :293-392; kernel :1795-1848) by one launch each way.
 *   alphas, t [S]; rgb [S,3] or NULL; ray_index int64 [P] or NULL: per-ray results go to element ray_index[p]
 *   (rays_inds_hit) of mask / depth [num_rays] / rgb_out [num_rays,3] (caller ZERO-INITs them when ray_index is given).
 *   vw [S] fully written, bit-identical to nr3d_alpha_to_vw_forward.  depth = sum(vw*t) / (mask + 1e-10) when
 *   normalize_depth, else sum(vw*t). */
int nr3d_pack_composite_fwd(uint32_t P, const float *alphas, const float *t, const float *rgb, const int64_t *pack_infos,
                            const int64_t *ray_index, float early_stop_eps, float alpha_thre, int normalize_depth,
                            float *vw, float *mask, float *depth, float *rgb_out, void *stream);
/* backward of the above: g_mask / g_depth [num_rays], g_rgb [num_rays,3], g_vw [S] (each may be NULL = zero);
 * mask, depth = the forward's outputs.  grad_alphas [S] fully written; grad_t [S], grad_rgb [S,3] optional. */
int nr3d_pack_composite_bwd(uint32_t P, const float *alphas, const float *vw, const float *t, const float *rgb,
                            const int64_t *pack_infos, const int64_t *ray_index, float early_stop_eps, float alpha_thre,
                            int normalize_depth, const float *mask, const float *depth, const float *g_mask,
                            const float *g_depth, const float *g_rgb, const float *g_vw, float *grad_alphas,
                            float *grad_t, float *grad_rgb, void *stream);
/* -------------------------------------------------------------------------------------------------
 * Ray-query glue (csrc/ray_glue.hip): the device-side steps between march, density query, pruning and composite that the
 * reference runs as chains of ATen ops with host syncs in between.  No single reference kernel each; cited per entry.
 * ---------------------------------------------------------------------------------------------- */
/* alpha = 1 - exp(-sigma * delta)  (nr3d_lib/graphics/nerf/nerf_utils.py:23-24 applied to sigma * deltas,
 * nerf_ray_query.py:126,178) and its gradient grad_sigma = grad_alpha * delta * exp(-sigma * delta).  [S] each. */
int nr3d_tau_to_alpha_fwd(uint64_t S, const float *sigma, const float *delta, float *alpha, void *stream);
int nr3d_tau_to_alpha_bwd(uint64_t S, const float *sigma, const float *delta, const float *grad_alpha, float *grad_sigma,
                          void *stream);
/* Visibility pruning (nr3d_lib/graphics/nerf/nerf_utils.py:64-98 packed_volume_render_compression + the index gathers
 * of nerf_ray_query.py:128-137).  counts int64 [P] = kept samples per pack (nr3d_alpha_to_vw_forward's num_steps):
 * begin_all [P] = new begin of EVERY pack; the packs that keep >= 1 sample, ascending: idx_out [P'] (tag[i] if tag is
 * given, else i) and pack_infos_out int64 [P', 2]; totals int64 [2] = {kept samples, P'}. */
int nr3d_prune_compact_packs(uint32_t P, const int64_t *counts, const int64_t *tag, int64_t *begin_all, int64_t *idx_out,
                             int64_t *pack_infos_out, int64_t *totals, void *scan_tmp, void *stream);
/* ... then the kept samples (selector uint8 [S], pack_infos = the un-pruned packs) move to their compact positions,
 * ascending inside a pack: pidx int64 [S'] = their old indices, and up to four per-sample arrays are gathered in the same
 * pass: f1, f2 float [S], f3 float [S, 3], l1 int64 [S] (each in/out pair optional). */
int nr3d_prune_compact_samples(uint32_t P, const int64_t *pack_infos, const int64_t *begin_all, const uint8_t *selector,
                               const float *f1, const float *f2, const float *f3, const int64_t *l1, int64_t *pidx,
                               float *f1_out, float *f2_out, float *f3_out, int64_t *l1_out, void *stream);
/* mark_pack_boundaries_cuda (:2765-2805): boundaries int32 [num]. */
int nr3d_mark_pack_boundaries(uint64_t num, int dtype, const void *pack_ids, int32_t *boundaries, void *stream);

/* octree_mark_consecutive_segments (pack_ops.cpp:58, pack_ops_cuda.cu:2807-2887): pidx int32 [n] = octree nodes hit by
 * every ray in order (packs = rays), point_hierarchies int16 [n_nodes,3]; mark_start / mark_end uint8 [n] ZERO-INIT:
 * first / last node of every run of face-adjacent nodes. */
int nr3d_octree_mark_consecutive_segments(uint32_t P, const int32_t *pidx, const int64_t *pack_infos,
                                          const int16_t *point_hierarchies, uint8_t *mark_start, uint8_t *mark_end,
                                          void *stream);

/* Spatial order of a batch of sample positions (ABI 5; csrc/ray_glue.hip): x float [n, 3] -> order int32 [n], order[k] = the sample
 * at position k of a Morton curve through a 2^bits_per_dim grid over the batch's own bounding box (ties in input order).  The
 * ray-query driver (graphics/nerf/nerf_ray_query.py) runs the field on the rendered samples in this order: samples of neighbouring
 * rays that share grid cells become consecutive lanes, which the LoTD backward merges before its scatter and the forward's
 * gathers coalesce (the reference has no counterpart: nerf_ray_query.py:140-160 queries in ray order).  bits_per_dim 1..10;
 * tmp: nr3d_spatial_order_tmp_bytes(n) bytes. */
uint64_t nr3d_spatial_order_tmp_bytes(uint32_t n);
int nr3d_spatial_order(uint32_t n, const float *x, uint32_t bits_per_dim, int32_t *order, void *tmp, void *stream);
/* the field's inputs in that order: x_out[k] = x[order[k]], ridx_out[k] = ridx[order[k]] (int64 ray index per sample, optional) and
 * dirs_out[k] = dirs[ridx[order[k]]] (per-RAY float [n_rays, 3], optional: the view_dirs[ridx] gather of nerf_ray_query.py:78) */
int nr3d_order_gather_inputs(uint32_t n, const int32_t *order, const float *x, const int64_t *ridx, const float *dirs, float *x_out,
                             int64_t *ridx_out, float *dirs_out, void *stream);
/* rows of up to two per-sample float arrays (a [n, wa], b [n, wb]; a width of 0 skips one) between the two orders:
 * scatter != 0: out[order[k]] = in[k] (the field's outputs back to the samples' own order); else out[k] = in[order[k]] */
int nr3d_order_move_rows(uint32_t n, const int32_t *order, int scatter, const float *a, uint32_t wa, float *a_out, const float *b,
                         uint32_t wb, float *b_out, void *stream);

/* The library's own point sort (csrc/rsort.hip, ABI 5), exported for its tests -- lotd_sorted.hip orders the points of a large-table
 * dL/dparam pass with it (the reference's default build has no library sort either: pack_ops_cuda.cu:2621-2629 compiles thrust
 * out, :2634-2720 is its own kernel).  Stable LSD radix sort of `batch` (1 or 2) independent arrays of (uint32 key, uint32
 * value) pairs of the same length by key bits [0, bits): kin{0,1} / vin{0,1} -> kout{0,1} / vout{0,1} (the second set ignored
 * for batch 1).  vin NULL: the values are the element indices.  n_dev (optional): element count in DEVICE memory, <= n_max.
 * Inputs are left untouched, outputs must not alias them; tmp: nr3d_sort_pairs_u32_tmp_bytes(n_max, batch) bytes. */
uint64_t nr3d_sort_pairs_u32_tmp_bytes(uint32_t n_max, int batch);
int nr3d_sort_pairs_u32(void *tmp, int batch, const uint32_t *kin0, const uint32_t *vin0, uint32_t *kout0, uint32_t *vout0,
                        const uint32_t *kin1, const uint32_t *vin1, uint32_t *kout1, uint32_t *vout1, uint32_t n_max,
                        const uint32_t *n_dev, int bits, void *stream);

/* =================================================================================================
 * Permutohedral-lattice encoder (ABI 11) -- replaces nr3d_lib.bindings._permuto
 *   pybind surface   csrc/permuto/src/permuto.cpp:30-75
 *   host API         csrc/permuto/include/permuto/permuto.h:87-180, csrc/permuto/src/permuto_cuda.cu
 *   kernels          csrc/permuto/include/permuto/permuto_cuda.h:124-1030
 * ============================================================================================== */
#define NR3D_PERMUTO_MAX_LEVELS 24
#define NR3D_PERMUTO_MAX_PSEUDO 512       /* n_encoded_dims <= 1024, pseudo levels of >= 2 features */
#define NR3D_PERMUTO_N_SUPPORTED_DIMS 27

typedef struct nr3d_permuto_meta {
	double level_scales0[NR3D_PERMUTO_MAX_LEVELS];        /* res_list */
	uint32_t level_n_feats[NR3D_PERMUTO_MAX_LEVELS];
	uint32_t level_n_params[NR3D_PERMUTO_MAX_LEVELS];     /* hashmap_size * n_feats */
	uint32_t level_offsets[NR3D_PERMUTO_MAX_LEVELS + 1];  /* elements, inside one table set */
	uint32_t level_sizes[NR3D_PERMUTO_MAX_LEVELS];        /* hashmap_size (entries) */
	uint32_t level_cols[NR3D_PERMUTO_MAX_LEVELS];         /* first output column of each level (no reference field) */
	uint16_t map_levels[NR3D_PERMUTO_MAX_PSEUDO];         /* level of each pseudo level */
	uint16_t map_cnt[NR3D_PERMUTO_MAX_PSEUDO];            /* index of the pseudo level inside its level */
	uint32_t n_levels;
	uint32_t n_pseudo_levels;
	uint32_t n_feat_per_pseudo_lvl;  /* 4 if every width divides by 4, else 2 */
	uint32_t n_dims_to_encode;
	uint32_t n_encoded_dims;
	uint32_t n_params;               /* == level_offsets[n_levels] */
} nr3d_permuto_meta_t;

/* supported_n_input_dims (permuto_cuda.cu:44): writes NR3D_PERMUTO_N_SUPPORTED_DIMS values into dims (if not NULL), returns their number */
int nr3d_permuto_supported_n_input_dims(int32_t *dims);
/* PermutoEncMeta::create_meta (permuto_cuda.cu:46-150).  Host only.  level_scales_multidim: optional host float [n_levels, n_input_dim]
 * out, res / sqrt((d+1)(d+2)) computed in double.  Errors: unsupported n_input_dim, n_levels > 24, a width not divisible by 2,
 * more than UINT32_MAX / 2 parameters, more than 1024 encoded dims. */
int nr3d_permuto_meta_create(int32_t n_input_dim, int32_t hashmap_size, uint32_t n_levels, const double *res_list,
                             const int32_t *n_feats_list, nr3d_permuto_meta_t *out, float *level_scales_multidim);

/* Common arguments (permuto_cuda.cu:152-526):
 *   x             float [N, D] contiguous (already multiplied by pos_scale)
 *   params        param_dtype (NR3D_F32 | NR3D_F16) 1-D: one or more table sets of n_params elements
 *   level_scales  DEVICE float [n_levels, D] (the meta's level_scales_multidim); level_random_shifts DEVICE float [n_levels, D] or NULL
 *   batch_inds    int64 [N] or NULL (< 0: point skipped, its outputs 0); batch_offsets int64 [B] or NULL (element offset of each
 *                 table set, a multiple of n_feat_per_pseudo_lvl; default b * n_params); batch_data_size > 0: b = i / batch_data_size
 *   max_level     levels > max_level contribute 0; <= -1: nothing is launched (the bindings return zeros / None)
 *   strides in ELEMENTS; dL_dy has the params dtype.
 * fp16 tables are read as half and used as float; y and dL_ddLdy are fp32 sums rounded once to half; dL_dparam is always fp32. */

/* permuto_enc_fwd: y[i*y_sn + e*y_se] (params dtype), fully written (skipped levels / points: 0). */
int nr3d_permuto_fwd(const nr3d_permuto_meta_t *meta, uint32_t n_points, int param_dtype, const float *x, const void *params,
                     const float *level_scales, const float *level_random_shifts, const int64_t *batch_inds,
                     const int64_t *batch_offsets, uint32_t batch_data_size, int32_t max_level, void *y, int64_t y_sn, int64_t y_se,
                     void *stream);
/* permuto_enc_bwd: dL_dx float [N, D] contiguous, fully written (columns >= max_pos_dims and skipped points: 0), or NULL;
 * dL_dparam float, numel of params, ZERO-INIT by the caller (hardware f32 atomics), or NULL. */
int nr3d_permuto_bwd(const nr3d_permuto_meta_t *meta, uint32_t n_points, int param_dtype, const void *dL_dy, int64_t dldy_sn,
                     int64_t dldy_se, const float *x, const void *params, const float *level_scales, const float *level_random_shifts,
                     const int64_t *batch_inds, const int64_t *batch_offsets, uint32_t batch_data_size, int32_t max_level,
                     uint32_t max_pos_dims, float *dL_dx, float *dL_dparam, void *stream);
/* permuto_enc_bwd_bwd_input: from dL_ddLdx float [N, D] contiguous to dL_ddLdy (params dtype, [i*sn + e*se], fully written, or NULL)
 * and dL_dparam (float, ZERO-INIT, or NULL).  x receives no second-order gradient (as in the reference). */
int nr3d_permuto_bwd_bwd_input(const nr3d_permuto_meta_t *meta, uint32_t n_points, int param_dtype, const float *dL_ddLdx,
                               const void *dL_dy, int64_t dldy_sn, int64_t dldy_se, const float *x, const void *params,
                               const float *level_scales, const float *level_random_shifts, const int64_t *batch_inds,
                               const int64_t *batch_offsets, uint32_t batch_data_size, int32_t max_level, void *dL_ddLdy,
                               int64_t ddldy_sn, int64_t ddldy_se, float *dL_dparam, void *stream);

/* =================================================================================================
 * Sphere tracer (ABI 14) -- replaces nr3d_lib.bindings._sphere_trace
 *   pybind surface   csrc/sphere_trace/src/entry.cu:14-47
 *   segment march    csrc/sphere_trace/include/sphere_trace/dense_grid.cuh:38-67,117-200, csrc/sphere_trace/src/ray_march.cu:11-129
 *   tracer           csrc/sphere_trace/src/sphere_tracer.cu:11-121,177-399, include/sphere_trace/sphere_tracer.cuh
 * Common arguments: rays_o / rays_d float [n_rays, 3], rays_near / rays_far float [n_rays], all contiguous; grid_occ bool (one byte)
 * [res0, res1, res2] over [-1, 1]^3; segs float [n_segs, 2] (t_enter, t_exit).  Status codes: ALIVE 0, HIT 1, OUT 2.
 * The tracer's state is a structure of arrays inside ONE caller-allocated block of nr3d_sphere_trace_state_bytes(cap) bytes per
 * buffer side (the caller keeps two and swaps them at every compaction), the hit list one block of nr3d_sphere_trace_hits_bytes(cap)
 * bytes; cap = the number of rays given to nr3d_sphere_trace_init, the same in every later call.  Neither needs initialising.  tmp:
 * nr3d_sphere_trace_tmp_bytes(n) bytes of device scratch.  `totals` / `total`: int64 words the last kernel stores with system scope
 * (pinned host memory + nr3d_wait_host_words, or device memory).  n == 0 is an ordinary input everywhere: nothing is launched, totals
 * are zeroed.  Not ported: the segs_endpoint_distances variant of init / advance and the debug outputs of ray_march. */
uint64_t nr3d_sphere_trace_state_bytes(uint32_t cap);
uint64_t nr3d_sphere_trace_hits_bytes(uint32_t cap);
uint64_t nr3d_sphere_trace_tmp_bytes(uint32_t n);
/* ray_march phase 1 + the compaction of the rays with >= 1 segment: valid_rays_idx int64 [n_rays] (the first totals[1] rows written,
 * ascending), pack_infos int64 [n_rays, 2] (begin, count) of those rays (same rows), totals = {segments, valid rays}. */
int nr3d_sphere_trace_march_count(uint32_t n_rays, const float *rays_o, const float *rays_d, const float *rays_near,
                                  const float *rays_far, const int32_t grid_res[3], const uint8_t *grid_occ, int64_t *valid_rays_idx,
                                  int64_t *pack_infos, int64_t *totals, void *tmp, void *stream);
/* ray_march phase 2 over the n_valid compacted rays: segs_pack_info int32 [n_valid, 2] (offset, count), segs float [total_segs, 2],
 * segs_endpoints float [total_segs, 2, 3] or NULL; all fully written. */
int nr3d_sphere_trace_march_write(uint32_t n_valid, const float *rays_o, const float *rays_d, const float *rays_near,
                                  const float *rays_far, const int32_t grid_res[3], const uint8_t *grid_occ,
                                  const int64_t *valid_rays_idx, const int64_t *pack_infos, int64_t total_segs, int32_t *segs_pack_info,
                                  float *segs, float *segs_endpoints, void *stream);
/* init_rays: n rows of (valid_rays_idx int64, segs_pack_info int32 [n, 2]) -> state rows [0, n), query positions included.  A row with
 * a ray index outside [0, n_rays), an empty pack or one outside [0, n_segs) starts as OUT. */
int nr3d_sphere_trace_init(uint32_t n, uint32_t n_rays, int64_t n_segs, const float *rays_o, const float *rays_d,
                           const int64_t *valid_rays_idx, const int32_t *segs_pack_info, const float *segs, void *state, uint32_t cap,
                           void *stream);
/* advance_rays: one step of the n buffered rays from distances float [n] (rows that are not ALIVE are left alone), and the next query
 * positions (inside the state block) in the same launch.  A non-finite distance ends its ray as OUT. */
int nr3d_sphere_trace_advance(uint32_t n, const float *rays_o, const float *rays_d, const float *distances, const float *segs, void *state,
                              uint32_t cap, float zero_offset, float distance_scale, float min_step, float hit_threshold, void *stream);
/* compact_rays: ALIVE rows of state_in move to state_out in their order, HIT rows are appended to hits at row n_hit in their order;
 * totals = {alive rows, new hits}. */
int nr3d_sphere_trace_compact(uint32_t n, void *state_in, void *state_out, uint32_t cap, void *hits, uint32_t n_hit, int64_t *totals,
                              void *tmp, void *stream);
/* get_rays(HIT) / get_rays(ALIVE): pos, dir float [n, 3], idx int64 [n], t float [n], n_steps int32 [n]; ALIVE also status uint8,
 * debug_flag int8, hit_region_infos float [n, 4], hit_seg_regions int32 [n, 2], seg_idxs / seg_end_idxs int32 [n]; fully written. */
int nr3d_sphere_trace_gather_hit(uint32_t n_hit, const float *rays_o, const float *rays_d, const void *hits, uint32_t cap, float *pos,
                                 float *dir, int64_t *idx, float *t, int32_t *n_steps, void *stream);
int nr3d_sphere_trace_gather_alive(uint32_t n, const float *rays_o, const float *rays_d, const void *state, uint32_t cap, float *pos,
                                   float *dir, int64_t *idx, float *t, int32_t *n_steps, uint8_t *status, int8_t *debug_flag,
                                   float *hit_region_infos, int32_t *hit_seg_regions, int32_t *seg_idxs, int32_t *seg_end_idxs,
                                   void *stream);
/* sample_on_segments phase 1 + the scan: pack_info int32 [n, 2] (offset, count), total[0] = samples; phase 2: samples_offset /
 * n_samples int32 [n], sample_depths float [total], sample_positions float [total, 3]; fully written. */
int nr3d_sphere_trace_sample_count(uint32_t n, float step_size, const float *segs, const void *state, uint32_t cap, int32_t *pack_info,
                                   int64_t *total, void *tmp, void *stream);
int nr3d_sphere_trace_sample_write(uint32_t n, float step_size, const float *rays_o, const float *rays_d, const float *segs,
                                   const void *state, uint32_t cap, const int32_t *pack_info, int64_t total, int32_t *samples_offset,
                                   int32_t *n_samples, float *sample_depths, float *sample_positions, void *stream);
/* trace_on_samples: the first (d >= 0, d <= 0) bracket of every buffered ray's samples becomes a hit, appended at row n_hit in the
 * rays' order (n_hit + n <= cap); totals = {0, new hits}. */
int nr3d_sphere_trace_trace_on_samples(uint32_t n, const void *state, uint32_t cap, const int32_t *samples_offset,
                                       const int32_t *n_samples, int64_t total, const float *sample_depths,
                                       const float *sample_distances, void *hits, uint32_t n_hit, int64_t *totals, void *tmp,
                                       void *stream);

/* =================================================================================================
 * Embedders -- replace nr3d_lib.bindings._shencoder and nr3d_lib.bindings._freqencoder
 *   pybind surfaces   externals/shencoder/bindings.cpp, externals/freqencoder/bindings.cpp
 *   kernels           externals/shencoder/shencoder.cu, externals/freqencoder/freqencoder.cu
 * Element-wise, one launch each, no workspace, no atomics, no host wait.  B == 0 is a no-op.
 * ============================================================================================== */

/* Real spherical harmonics of x [B, 3] as polynomials on all of R^3 (no normalisation): y[b, l*l + l + m], l < degree, degree 1..8,
 * D must be 3.  dtype NR3D_F32 or NR3D_F16 for every tensor of the call; arithmetic in fp32, one rounding at the store.
 * y: rows of degree^2 elements, y_stride elements apart (>= degree^2: a column slice of a wider row-major buffer is a valid output; the
 * other columns are not touched).  dy_dx: NULL, or [B, 3, degree^2] (the reference's layout) to also store the Jacobian. */
int nr3d_sh_encode_fwd(uint64_t B, uint32_t D, uint32_t degree, int dtype, const void *x, void *y, int64_t y_stride, void *dy_dx, void *stream);
/* grad_x[b, d] = sum_c grad[b, c] dY_c/dx_d (accumulate != 0: added to what grad_x holds).  dy_dx == NULL: the derivatives are
 * recomputed from x; otherwise they are read from the stored Jacobian and x may be NULL.  grad rows grad_stride elements apart. */
int nr3d_sh_encode_bwd(uint64_t B, uint32_t D, uint32_t degree, int dtype, const void *grad, int64_t grad_stride, const void *x,
                       const void *dy_dx, void *grad_x, int accumulate, void *stream);

/* Sinusoidal embedding of x [B, D], float32, D >= 1, C = D + 2 D n_freq, n_freq <= 24 (from f = 24 on, 2^f x + pi/2 has no phase left
 * in fp32), B * C < 2^31: y[b, c] = x[b, c] for c < D, else sin(2^f x[b, d] + k pi/2) with col = c / D - 1, d = c % D, f = col / 2,
 * k = col % 2, the argument formed in fp32.  y rows y_stride (>= C) elements apart. */
int nr3d_freq_encode_fwd(uint64_t B, uint32_t D, uint32_t n_freq, uint32_t C, const float *x, float *y, int64_t y_stride, void *stream);
/* grad_x [B, D] (overwritten) from grad [B, C] and the forward's outputs y, no trigonometry:
 * grad_x[d] = g[d] + sum_f 2^f (g[f,0,d] y[f,1,d] - g[f,1,d] y[f,0,d]). */
int nr3d_freq_encode_bwd(uint64_t B, uint32_t D, uint32_t n_freq, uint32_t C, const float *grad, const float *y, int64_t y_stride,
                         float *grad_x, void *stream);
/* The backward of nr3d_freq_encode_bwd.  v = dL/d(grad_x) [B, D]; outputs, each optional (NULL) and overwritten:
 * d_grad [B, C] = dL/dgrad:  v[d];  v[d] 2^f y[f,1,d];  -v[d] 2^f y[f,0,d]
 * d_x [B, D]    = dL/dx:     -v[d] sum_f 4^f (g[f,0,d] y[f,0,d] + g[f,1,d] y[f,1,d])      (needs grad). */
int nr3d_freq_encode_bwd_bwd(uint64_t B, uint32_t D, uint32_t n_freq, uint32_t C, const float *v, const float *grad, const float *y,
                             int64_t y_stride, float *d_grad, float *d_x, void *stream);

/* =================================================================================================
 * NeuS coarse ray query: one up-sampling stage on fixed-length rows in one launch
 *   reference         the torch op chain of nr3d_lib/graphics/neus/neus_ray_query.py:258-270 (neus_ray_sdf_to_alpha |
 *                     neus_ray_sdf_to_upsample_alpha, ray_alpha_to_vw, batch_sample_pdf, cat, sort); no native twin there
 * One 64-lane wave per ray, the row staged in LDS; no workspace, no atomics, no host wait; the same bits run after run.
 * ============================================================================================== */

/* Rows of n + m elements up to this cap are served (the default four stages of 64 + 65 end at 325). */
#define NR3D_NEUS_UPSAMPLE_MAX_ROW 1024
int nr3d_neus_upsample_max_row(void);

/* For each of R rays: depth, sdf [R, n] float32 (n >= 2; depth non-decreasing per row) are the interval boundaries and the SDF there.
 * Interval opacity alpha_i, i < n - 1:
 *   use_estimate == 0: c = sigmoid(sdf inv_s), alpha_i = max(0, (c_i - c_{i+1}) / (c_i + 1e-5));
 *   use_estimate != 0: delta_i = depth_{i+1} - depth_i, mid_i = (sdf_i + sdf_{i+1}) / 2, slope_i = (sdf_{i+1} - sdf_i) / (delta_i + 1e-5),
 *     s_i = clamp(min(slope_{i-1}, slope_i), -10, 0) with slope_{-1} = 0, c_prev|c_next = sigmoid((mid_i -|+ s_i delta_i / 2) inv_s),
 *     alpha_i = max(0, (c_prev - c_next) / (c_prev + 1e-5)).
 * Weights w_i = alpha_i prod_{j<i} (1 - alpha_j); cdf_0 = 0, cdf_{i+1} = cdf_i + w_i / max(sum w, 1e-5).
 * u: the CDF positions to invert, m >= 1 per row, non-decreasing; row r starts at u + r * u_stride, u_stride 0 (one shared row) or m.
 * For every u_j: k = the first index with cdf_k >= u_j (n if none), lo = max(k - 1, 0), hi = min(k, n - 1), den = cdf_hi - cdf_lo (1 where
 * below 1e-5), fine_j = depth_lo + (u_j - cdf_lo) / den * (depth_hi - depth_lo), then raised to the running maximum of the row (a no-op
 * wherever that expression is monotone, which it is up to its last rounding).
 * Outputs, fully written: fine [R, m]; merged [R, n + m] = the sorted union of the row's depth and fine; order int32 [R, n + m] = the
 * position in cat(depth, fine) every merged element came from, depth elements first among equal values.
 * n + m <= NR3D_NEUS_UPSAMPLE_MAX_ROW, otherwise an error before any launch.  R == 0 is a no-op. */
int nr3d_neus_upsample_stage(uint32_t R, uint32_t n, uint32_t m, const float *depth, const float *sdf, const float *u, int64_t u_stride,
                             float inv_s, int use_estimate, float *fine, float *merged, int32_t *order, void *stream);

/* -------------------------------------------------------------------------------------------------
 * The same stage on the packs of a marcher: the up-sampling of neus_ray_query_march_occ_multi_upsample[_compressed], and with a label
 * per sample of the forest's march-occ queries, in one launch
 *   reference         the packed op chain of nr3d_lib/graphics/neus/neus_ray_query.py (neus_packed_sdf_to_alpha |
 *                     neus_packed_sdf_to_upsample_alpha, packed_alpha_to_vw, packed_cumsum, packed_div, packed_sample_cdf,
 *                     merge_two_packs_sorted_aligned and the index-puts of the driver); no native twin there
 * One 64-lane wave per pack, four packs per workgroup, no workgroup barrier; no atomics, no host wait; every output element is written
 * once by a fixed lane, so the result is the same bits run after run.
 * ------------------------------------------------------------------------------------------------- */

/* Packs with len + m up to this are staged in LDS (4 * 3 * this many floats per workgroup); longer ones run the same code on global
 * memory with the CDF in the caller's workspace.  A compile-time choice (-DNR3D_NEUS_UPSAMPLE_PACKED_LDS_ROW=256|512|1024). */
#ifndef NR3D_NEUS_UPSAMPLE_PACKED_LDS_ROW
#define NR3D_NEUS_UPSAMPLE_PACKED_LDS_ROW 512
#endif
int nr3d_neus_upsample_packed_lds_row(void);

/* depth, sdf float32 [N], packed: pack p holds the len_p elements from first_p on, pack_infos int64 [P, 2] = (first_p, len_p); depth is
 * non-decreasing inside a pack.
 * PRECONDITION: the packs tile [0, N) in order -- first_0 = 0, first_{p+1} = first_p + len_p, len_p >= 1 -- which is what every marcher
 * of this library returns for its hit rays.  The layout of the outputs relies on it; a pack_infos that breaks it makes packs overlap
 * in the outputs, but no access leaves the buffers (a pack is clipped to [0, N), and one without elements gets fine = 0).
 * Per pack, with n = len_p (the last element of a pack closes no interval: alpha_{n-1} = 0):
 *   opacity, use_estimate == 0 (neus_packed_sdf_to_alpha): c = sigmoid(sdf inv_s), alpha_i = max(0, (c_i - c_{i+1}) / (c_i + 1e-5));
 *   use_estimate != 0 (neus_packed_sdf_to_upsample_alpha): dsdf_i = sdf_{i+1} - sdf_i, delta_i = depth_{i+1} - depth_i,
 *     slope_i = dsdf_i / (delta_i + 1e-5), s_i = clamp(min(slope_{i-1}, slope_i), -10, 0) with slope_{-1} = 0, mid_i = sdf_i + dsdf_i / 2,
 *     half_i = s_i delta_i / 2, c_prev|c_next = sigmoid((mid_i -|+ half_i) inv_s), alpha_i = max(0, (c_prev - c_next) / (c_prev + 1e-5));
 *   weights (packed_alpha_to_vw, early_stop_eps 1e-4, alpha_thre 0): T_i = prod_{j<i, alpha_j > 0} (1 - alpha_j); w_i = alpha_i T_i while
 *     T_i >= 1e-4, w_i = 0 from the first T_i < 1e-4 on (the product associates as a scan tree);
 *   cdf_i = (sum_{j<i} w_j) / max(sum_{j<n-1} w_j, 1e-5): summed first, divided afterwards;
 *   inversion (packed_invert_cdf) at u_j: pos = min(first k with cdf_k >= u_j, n - 1); pos == 0 -> depth_0; else pmf = cdf_pos - cdf_{pos-1},
 *     pmf < 1e-5 -> depth_{pos-1}, otherwise fmaf((u_j - cdf_{pos-1}) / pmf, depth_pos - depth_{pos-1}, depth_{pos-1}); then raised to the
 *     running maximum over j (a no-op wherever the expression is monotone in u).  A pack of one element therefore gives depth_0 and
 *     one without mass depth_{n-2}, for every u.
 * u: m >= 1 CDF positions per pack, non-decreasing; pack p reads u + p * u_stride, u_stride 0 (one shared row) or m.
 * Outputs, fully written: fine [P, m].  With merge != 0 also merged [N + P m]: pack p starts at first_p + p m and is the sorted union of
 * its depths and its new depths, a new depth BEFORE an old one of equal value and equal new depths in their order
 * (merge_two_packs_sorted_aligned); pack_infos_out int64 [P, 2] = (first_p + p m, len_p + m); pidx_fine int64 [P, m] = the index in
 * merged of every new depth.  With need_sdf != 0 (needs merge) sdf_merged [N + P m] holds every old SDF value at its depth's index in
 * merged; the elements at pidx_fine are NOT written, the caller fills them with the SDF at the new depths.
 * cdf_workspace: float32 [N], contents undefined on return; always required (packs longer than the LDS row keep their CDF there).
 * Labels, optional: blidx int64 [N] gives every sample a label -- the block index of a forest's samples (the up-sampling of the
 * reference's NeuSRendererMixinForest, nr3d_lib/models/fields_forest/neus/renderer_mixin.py: `blidx[pidx_fine_iter]` and the index-puts
 * of blidx); any value, nothing interprets it.  blidx == NULL runs the stage without labels, and blidx_fine and blidx_merged must be
 * NULL too; with blidx, blidx_fine is required, and so is blidx_merged with merge != 0.  The other outputs are the same bits either way.
 *   blidx_fine int64 [P, m], fully written: blidx_fine[p, j] = blidx[first_p + pos_j], pos_j the inversion's own pos -- the upper end
 *     of the bin, packed_invert_cdf's bin index -- taken before fine_j is raised to the running maximum and whether or not that raise
 *     changes it.  A pack without elements (outside the contract) gets -1.
 *   blidx_merged int64 [N + P m], fully written with merge != 0: an old depth's place holds its old label,
 *     blidx_merged[pidx_fine[p, j]] = blidx_fine[p, j].
 *   Labels are not staged in LDS (the workgroup's footprint is the same with and without them): blidx is read once per new depth and
 *   once per old element of the union.
 * Unused outputs may be NULL.  m >= 1, u_stride in {0, m}, N + P m < 2^31, need_sdf only with merge and the label rules above, otherwise
 * an error before any launch.  P == 0 is a no-op. */
int nr3d_neus_upsample_stage_packed(uint32_t P, uint64_t N, uint32_t m, const float *depth, const float *sdf, const int64_t *blidx,
                                    const int64_t *pack_infos, const float *u, int64_t u_stride, float inv_s, int use_estimate, int merge,
                                    int need_sdf, float *cdf_workspace, float *fine, int64_t *blidx_fine, float *merged,
                                    float *sdf_merged, int64_t *blidx_merged, int64_t *pidx_fine, int64_t *pack_infos_out, void *stream);

/* =================================================================================================
 * NeuS opacity: the SDF of consecutive samples -> alpha, one launch each way (csrc/neus_alpha.hip)
 *   reference         the torch op chain of nr3d_lib/graphics/neus/neus_utils.py:48-117 (neus_ray_sdf_to_alpha,
 *                     neus_packed_sdf_to_alpha: sdf * inv_s, sigmoid, diff | packed_diff, negate, + 1e-5, divide, clamp_min) and its
 *                     autograd; no native twin there
 *   c_i = sigmoid(sdf_i inv_s), alpha_i = max(0, (c_i - c_next) / (c_i + 1e-5)); c_next = the next sample of the same pack or row,
 *   for the last sample by append_mode: NONE -- no interval, alpha = 0 (packed) / no output element (rows); ONE -- c_next = 1;
 *   SDF (packed only) -- c_next = sigmoid(pack_sdf_appends[p] inv_s), pack_sdf_appends float32 [P].
 * layout PACKED: sdf [S], pack_infos int64 [P, 2] = (first, len), alpha [S]; n is ignored.  One wave per pack; a pack is clipped to
 *   [0, S); zero-length packs are allowed; rows outside every pack are 0: ordered_packs as for nr3d_packed_diff (!= 0: the kernel zeroes
 *   them itself, the outputs may be uninitialised; == 0: pass zeroed alpha / grad_sdf).
 * layout ROWS: sdf [P, n] (S = P n, n >= 1; pack_infos NULL, ordered_packs ignored), alpha [P, n_out], n_out = n - 1 (NONE) or n (ONE),
 *   fully written; n_out == 0 launches nothing.
 * inv_s: read from inv_s_dev[0] (one float in device memory) when inv_s_dev != NULL, else the value inv_s.  No host wait either way.
 * S < 2^32.  fp32; the sigmoid as E = exp(-|z|), c = 1 / (1 + E) | E / (1 + E) by the sign of z, c' = E / (1 + E)^2.  The same data
 * gives the same bits in both layouts.
 * ============================================================================================== */
#define NR3D_NEUS_ALPHA_PACKED 0
#define NR3D_NEUS_ALPHA_ROWS 1
#define NR3D_NEUS_ALPHA_APPEND_NONE 0
#define NR3D_NEUS_ALPHA_APPEND_ONE 1
#define NR3D_NEUS_ALPHA_APPEND_SDF 2
int nr3d_neus_alpha_fwd(int layout, uint32_t P, uint64_t S, uint32_t n, const float *sdf, const int64_t *pack_infos, int append_mode,
                        const float *pack_sdf_appends, float inv_s, const float *inv_s_dev, int ordered_packs, float *alpha, void *stream);
/* The gradients, recomputed from the forward's inputs (nothing else is kept).  grad_alpha = dL/dalpha, alpha's shape.  With
 * m_i = [(c_i - c_next) / (c_i + 1e-5) >= 0] (the gradient passes at equality, as torch's clamp_min):
 *   u_i = c'_i (grad_alpha_i m_i (c_next + 1e-5) / (c_i + 1e-5)^2 - grad_alpha_{i-1} m_{i-1} / (c_{i-1} + 1e-5)), the second term inside
 *   the same pack or row only;  grad_sdf_i = inv_s u_i (sdf's shape; 0 outside the packs);  append_mode SDF: grad_appends [P] =
 *   inv_s u_append, u_append = -c'_append grad_alpha_last m_last / (c_last + 1e-5) (0 for a zero-length pack), else grad_appends is unused.
 * grad_inv_s (optional, one float in device memory) = sum_i sdf_i u_i + sum_p append_p u_append,p: WRITTEN, not accumulated.  Every
 *   workgroup writes one partial into `workspace` (nr3d_neus_alpha_bwd_workspace_bytes(layout, P, S) bytes, contents undefined on
 *   return) and a second launch of one workgroup adds them in a fixed order -- no float atomics, the same bits run after run.  Without
 *   grad_inv_s: one launch, no workspace. */
uint64_t nr3d_neus_alpha_bwd_workspace_bytes(int layout, uint32_t P, uint64_t S);
int nr3d_neus_alpha_bwd(int layout, uint32_t P, uint64_t S, uint32_t n, const float *sdf, const int64_t *pack_infos, int append_mode,
                        const float *pack_sdf_appends, float inv_s, const float *inv_s_dev, int ordered_packs, const float *grad_alpha,
                        float *grad_sdf, float *grad_appends, float *grad_inv_s, void *workspace, uint64_t workspace_bytes, void *stream);

/* =================================================================================================
 * NeuS render: the volume buffer -> vw, mask, depth, rgb and the rendered normal of every ray, one launch each way (csrc/neus_composite.hip)
 *   reference         the torch op chain at the end of NeusRendererMixin.ray_query (nr3d_lib/models/fields/neus/renderer_mixin.py:396-439:
 *                     ray_alpha_to_vw | packed_alpha_to_vw, then sum | packed_sum, div | packed_div, mul and index-put per output) and its
 *                     autograd; no native twin there
 * layout ROWS ('batched' buffers): alphas, t [P, n] (S = P n, n >= 1; pack_infos NULL), row r = samples [r n, (r + 1) n).  The semantics of
 *   ray_alpha_to_vw: w_i = a_i T_i, T_0 = 1, T_{i+1} = T_i (1 - a_i) over EVERY sample; early_stop_eps and alpha_thre are ignored.  G = the
 *   power of two >= n (at most 64) lanes work on a row; T is a prefix product, so vw equals the chain's up to rounding.
 * layout PACKED: alphas, t [S], pack_infos int64 [P, 2] = (first, len); n is ignored.  Forward and backward are those of
 *   nr3d_pack_composite_fwd / _bwd in every respect (early_stop_eps, alpha_thre with `<=` forward and `<` backward, the backward's
 *   max(1 - a, 1e-10) divisor, NR3D_OPT_PACK_SCAN and its serial replay of ambiguous packs), and without nablas the call is forwarded to
 *   them: the same bits.  With nablas one wave works on a pack at every pack count.
 * rgb [S, 3] or NULL; nablas [S, 3] or NULL, composited like rgb into normals_out by normals_mode:
 *   0 (training)    normals_out = sum_i w_i nablas_i;
 *   1 (evaluation)  normals_out = sum_i w_i c_i / max(|c_i|, 1e-12), c_i = clamp(nablas_i, -1, 1), and c_i is STORED BACK into nablas (the
 *                   reference's clamp_ is in place) for every sample of a row or pack; a zero vector contributes zero; forward only.
 * ray_index int64 [P] or NULL: the per-ray results go to element ray_index[p] of mask / depth [num_rays], rgb_out / normals_out
 *   [num_rays, 3], which the caller ZERO-INITs when ray_index is given.  depth = sum(w t) / (mask + 1e-10) when normalize_depth, else
 *   sum(w t).  vw [S] is fully written over the rows or packs; samples outside every pack are the caller's.
 * Errors before any launch: an unknown layout or normals_mode, rows with pack_infos or with n == 0 and P > 0 or P n != S, S >= 2^32,
 *   rgb / nablas without their output.  P == 0 is a no-op.  fp32; nothing is accumulated across waves: the same bits run after run.
 * ============================================================================================== */
#define NR3D_NEUS_COMPOSITE_ROWS 0
#define NR3D_NEUS_COMPOSITE_PACKED 1
int nr3d_neus_composite_fwd(int layout, uint32_t P, uint64_t S, uint32_t n, const float *alphas, const float *t, const float *rgb,
                            float *nablas, const int64_t *pack_infos, const int64_t *ray_index, float early_stop_eps, float alpha_thre,
                            int normalize_depth, int normals_mode, float *vw, float *mask, float *depth, float *rgb_out, float *normals_out,
                            void *stream);
/* The gradients.  vw, mask, depth = the forward's outputs; g_mask / g_depth [num_rays], g_rgb / g_normals [num_rays, 3], g_vw [S] (each may
 * be NULL = zero).  With g_i = dL/dw_i = g_mask + the depth term + g_rgb . rgb_i + g_normals . nablas_i + g_vw_i:
 *   ROWS    grad_alphas_i = T_i (g_i - R_i), R_i = g_{i+1} a_{i+1} + (1 - a_{i+1}) R_{i+1}, R_{n-1} = 0: the derivative of the product with
 *           the sample's own factor left out (torch's cumprod backward), no division -- exact where some a_i == 1;
 *   PACKED  as nr3d_pack_composite_bwd.
 * grad_alphas [S] fully written over the rows or packs; grad_t [S], grad_rgb [S, 3], grad_nablas [S, 3] = w_i g_normals optional (NULL:
 * not computed).  normals_mode 1 together with g_normals or grad_nablas is an error (the normalised normals are forward only); nablas is
 * read only where g_normals is given. */
int nr3d_neus_composite_bwd(int layout, uint32_t P, uint64_t S, uint32_t n, const float *alphas, const float *t, const float *rgb,
                            const float *nablas, const int64_t *pack_infos, const int64_t *ray_index, float early_stop_eps, float alpha_thre,
                            int normalize_depth, int normals_mode, const float *vw, const float *mask, const float *depth,
                            const float *g_mask, const float *g_depth, const float *g_rgb, const float *g_normals, const float *g_vw,
                            float *grad_alphas, float *grad_t, float *grad_rgb, float *grad_nablas, void *stream);

/* =================================================================================================
 * NeRF march + up-sample ray query: its two packed stages, one launch each (csrc/nerf_upsample.hip)
 *   reference         the torch op chains of nr3d_lib/graphics/nerf/nerf_ray_query.py:289-302 (merge_two_packs_sorted_a_includes_b, the
 *                     index-puts, addcmul, packed_diff) and :332-360 (tau_to_alpha, packed_cumsum, packed_div, packed_sample_cdf, the
 *                     second merge with its sort, packed_diff); no native twin there
 * One 64-lane wave per ray or pack, four per workgroup, no workgroup barrier; no atomics, no host wait; every output element is written
 * once by a fixed lane, so the result is the same bits run after run.
 * ============================================================================================== */

/* Rows up to this many elements are staged in LDS (4 * 2 * this many floats per workgroup, both kernels): num_coarse + len for the
 * merge, len + m + num_coarse for the stage; longer ones run the same code on global memory (the stage with its CDF in the caller's
 * workspace).  A compile-time choice (-DNR3D_NERF_UPSAMPLE_LDS_ROW=256|512|1024). */
#ifndef NR3D_NERF_UPSAMPLE_LDS_ROW
#define NR3D_NERF_UPSAMPLE_LDS_ROW 512
#endif
int nr3d_nerf_upsample_lds_row(void);

/* The union of every ray's coarse row with its marched pack.  coarse float32 [R, num_coarse] (non-decreasing per row, num_coarse >= 1);
 * depth float32 [N], the marched depths, non-decreasing inside a pack; pack_infos_all int64 [R, 2] = (first_r, len_r), the marched pack
 * of EVERY ray: len_r = 0 for a ray the marcher missed, and first_r = the sum of the lengths before r for all of them (the packs tile
 * [0, N) in ray order; a pack is clipped to [0, N), so no access leaves the buffers whatever it holds); rays_o, rays_d float32 [R, 3].
 * Outputs, fully written, [R num_coarse + N] each, ray r's pack starting at r num_coarse + first_r:
 *   depths_all  the sorted union of the row and the pack -- a marched depth BEFORE a coarse one of equal value, as
 *               try_merge_two_packs_sorted_aligned(a = coarse, b = marched) places them (the values are the same either way);
 *   deltas_all  packed_diff without appends: d[i+1] - d[i], 0 for the last element of a pack;
 *   ridx_all    int64, r;
 *   samples_all [., 3] = rays_o + rays_d t per component, the product rounded before the sum (what torch.addcmul computes);
 *   pack_infos_out int64 [R, 2] = (r num_coarse + first_r, num_coarse + len_r).
 * No arithmetic touches a depth but that subtraction, that product and that sum: every output equals the op chain's bit for bit.
 * N + R num_coarse < 2^31, otherwise an error before any launch.  R == 0 is a no-op. */
int nr3d_nerf_merge_rows_packs(uint32_t R, uint32_t num_coarse, uint64_t N, const float *coarse, const float *depth,
                               const int64_t *pack_infos_all, const float *rays_o, const float *rays_d, float *depths_all,
                               float *deltas_all, int64_t *ridx_all, float *samples_all, int64_t *pack_infos_out, void *stream);

/* One importance-resampling stage on the density.  depth, sigma, delta float32 [N], packed, pack_infos int64 [P, 2] = (first_p, len_p);
 * depth is non-decreasing inside a pack.  PRECONDITION: the packs tile [0, N) in order with len_p >= 1, as for
 * nr3d_neus_upsample_stage_packed; a pack is clipped to [0, N) and one without elements gets fine = 0.
 * Per pack of n elements, float32, in this order of operations:
 *   alpha_i = 1 - exp(-(sigma_i delta_i)), evaluated as -expm1(-(sigma_i delta_i)): the same quantity to full float32 precision, where
 *   the literal expression keeps a multiple of 2^-24 of a small optical depth;
 *   c_i = the inclusive sum of alpha up to i (it associates as a scan tree over chunks of 64);
 *   cdf_i = c_i / max(c_{n-1}, 1e-5): summed first, divided afterwards -- the CDF is the sum of the OPACITIES, not of weights, and has
 *   no leading zero;
 *   inversion (packed_invert_cdf) at u_j: pos = min(first k with cdf_k >= u_j, n - 1); pos == 0 -> depth_0; else pmf = cdf_pos - cdf_{pos-1},
 *     pmf < 1e-5 -> depth_{pos-1}, otherwise fmaf((u_j - cdf_{pos-1}) / pmf, depth_pos - depth_{pos-1}, depth_{pos-1}).  A pack of one
 *     element therefore gives depth_0 and one without mass depth_{n-2}, for every u;
 *   then fine_j is raised to the running maximum over j.  DEVIATION: the reference sorts the row instead (b_sorted = False in its second
 *     merge).  The two give the same values wherever the expression above is monotone in u, which it is up to the last rounding of
 *     the fma; where that rounding breaks the order by an ulp, the sort permutes two values and the maximum repeats the larger one.
 * u: m = num_fine + 1 >= 1 CDF positions per pack, non-decreasing; pack p reads u + p * u_stride, u_stride 0 (one shared row) or m.
 * Outputs, fully written: fine [P, m], and
 *   num_coarse > 0: coarse float32 [n_coarse_rows, num_coarse], non-decreasing per row; pack p takes row coarse_row[p] (int64 [P],
 *     clipped to the rows there are; NULL: row p).  merged [P, num_coarse + m] = the sorted union of that row and fine;
 *     deltas [P, num_coarse + m] = packed_diff of merged: the last column 0;
 *   num_coarse == 0: deltas [P, m - 1] = fine_{j+1} - fine_j and merged [P, m - 1] = fine_j + deltas_j.  This keeps the reference's own
 *     arithmetic (nerf_ray_query.py:357 adds the WHOLE difference, not half of it: the depths are the upper ends of the intervals).
 * cdf_workspace: float32 [N], contents undefined on return; always required (packs longer than the LDS row keep their CDF there).
 * m >= 1, u_stride in {0, m}, N < 2^31, P (m + num_coarse) < 2^31, otherwise an error before any launch.  P == 0 is a no-op. */
int nr3d_nerf_upsample_stage_packed(uint32_t P, uint64_t N, uint32_t m, uint32_t num_coarse, uint64_t n_coarse_rows, const float *depth,
                                    const float *sigma, const float *delta, const int64_t *pack_infos, const float *u, int64_t u_stride,
                                    const float *coarse, const int64_t *coarse_row, float *cdf_workspace, float *fine, float *merged,
                                    float *deltas, void *stream);

/* =================================================================================================
 * NeRF++ distant-view shell marcher: the samples of every ray on N (+ 1) concentric shells, packed, two launches (csrc/nerfpp_march.hip)
 *   reference         the torch op chain of NeRFRendererMixinDistant._ray_marching
 *                     (nr3d_lib/models/fields_distant/nerf/renderer_mixin.py:170-288, ray_sphere_intersect :31-50, ray_box_intersect
 *                     :53-82); no native twin there
 * rays_o, rays_d float32 [R, 3] in object space, t_min float32 [R]; aabb float32 [2, 3], READ ON THE DEVICE: c = (aabb[1] + aabb[0]) / 2,
 * h = (aabb[1] - aabb[0]) / 2, s = min_k (aabb[1] - aabb[0])_k; normalised ray o_n = (o - c) / h, d_n = d / h.
 * radii float32 [N] (N >= 1): the table of the chain's torch.arange; noise float32 [R, N] or NULL; step, last_radius floats.
 * Shell j < N of a ray, float32, in this order of operations:
 *   interval_type INVERSE:            r_reci = radii[j], with noise clamp_min(radii[j] + noise[ray, j] * step, 1e-5); r = 1 / r_reci
 *   LOGARITHM, LOGARITHM_INV_INPUT:   r_log = radii[j] (+ noise[ray, j] * step); r = powf(10, r_log); r_reci = 1 / r
 *   r_ext[j] = r[j], r_ext[N] = last_radius.
 *   sample_mode BOX:       t_ext = box(o_n, d_n, r_ext)        ELLIPSOID: t_ext = sphere(o_n, d_n, r_ext)
 *               CUBE:      t_ext = box(o, d, r_ext * s)        SPHERICAL: t_ext = sphere(o, d, r_ext * s)
 *     box(o, d, r):    a_k = (-r - o_k) / d_k, b_k = (r - o_k) / d_k; t_near = max_k min(a_k, b_k), t_far = min_k max(a_k, b_k), both
 *                      NaN-PROPAGATING as torch.minimum / maximum / max(dim) / min(dim) (a 0/0 slab term makes the shell invalid; the
 *                      infinities of a zero direction component are ordinary values); (t_far > t_near) & (t_far > 0) ? t_far : NaN
 *     sphere(o, d, r): pp = o.o, vv = d.d, pv = o.d; (sqrt(pv pv - vv (pp - r r)) - pv) / vv  (a negative discriminant gives NaN)
 *   t = t_ext[j], delta = t_ext[j + 1] - t_ext[j] (written even when it is NaN); the shell is valid iff !(isnan(t) | (t < t_min[ray]))
 *   -- exactly that boolean: a NaN t_min keeps the sample.
 *   network input x [4]:
 *     BOX, ELLIPSOID:   p = o_n + d_n t (one fma per component); x_0..2 = p r_reci; q = r_reci, l = r_log
 *     CUBE, SPHERICAL:  p = ((o + d t) - c) / h; n = |p|; x_0..2 = p / max(n, 1e-12); q = 1 / n, l = log10f(n)
 *     x_3 = q 2 - 1 (INVERSE, LOGARITHM_INV_INPUT) or (l - log_min) / (log_max - log_min) 2 - 1 (LOGARITHM).
 * nr3d_nerfpp_march_count: counts int64 [R] = the valid shells of every ray, fully written.  The caller turns them into begin_all
 *   (the exclusive sum) and the sample total S with nr3d_prune_compact_packs.
 * nr3d_nerfpp_march_emit: the same inputs and begin_all int64 [R]; the valid shells in (ray, shell) ascending order -- the order of the
 *   chain's nonzero() -- into x float32 [S, 4] (16-byte aligned), t float32 [S], deltas float32 [S], ridx int64 [S], each fully
 *   written when begin_all and S come from the count of the same inputs; no row >= S is ever written.
 * One wave per ray, lane = shell in chunks of 64, four rays per workgroup; a lane computes t_ext[j] and t_ext[j + 1] itself; position =
 * begin_all[ray] + the chunks before + the valid lanes below (ballot).  No LDS, no atomics.  R < 2^28 (nr3d_prune_compact_packs),
 * R N < 2^40; R == 0 is a no-op. */
enum { NR3D_NERFPP_BOX = 0, NR3D_NERFPP_ELLIPSOID = 1, NR3D_NERFPP_CUBE = 2, NR3D_NERFPP_SPHERICAL = 3 };
enum { NR3D_NERFPP_INVERSE = 0, NR3D_NERFPP_LOGARITHM = 1, NR3D_NERFPP_LOGARITHM_INV_INPUT = 2 };
int nr3d_nerfpp_march_count(uint32_t R, const float *rays_o, const float *rays_d, const float *t_min, const float *aabb, uint32_t N,
                            const float *radii, const float *noise, float step, float last_radius, int sample_mode, int interval_type,
                            float log_min, float log_max, int64_t *counts, void *stream);
int nr3d_nerfpp_march_emit(uint32_t R, const float *rays_o, const float *rays_d, const float *t_min, const float *aabb, uint32_t N,
                           const float *radii, const float *noise, float step, float last_radius, int sample_mode, int interval_type,
                           float log_min, float log_max, const int64_t *begin_all, uint64_t S, float *x, float *t, float *deltas,
                           int64_t *ridx, void *stream);

/* ---- marching cubes (csrc/marching_cubes.hip; no reference twin: the reference copies the SDF volume to the host and calls
 * skimage.measure.marching_cubes, nr3d_lib/graphics/trianglemesh.py:210-214).  The case table is csrc/mc_table.inc, written by
 * tools/gen_mc_table.py (corner c at offsets (c & 1, (c >> 1) & 1, (c >> 2) & 1); edge e = 4 axis + u + 2 v, owned by the node at its low
 * end).  volume float32 [Nx, Ny, Nz] contiguous, every dimension >= 2, Nx Ny < 2^28 rows, fewer than 2^36 nodes.
 *   A node is inside iff v < level, outside iff v >= level; NaN is neither.
 *   A cell (i, j, k), i < Nx - 1 ..., is ACTIVE iff its 8 corner values are finite; it emits its case's triangles (case = sum of
 *     inside(c) << c), an inactive cell emits nothing.  NaN marks nodes that were not evaluated; there is no mask argument.
 *   An edge is LIVE iff one end is inside and the other outside and at least one of its up to four incident cells is active.  One
 *     vertex per live edge and none otherwise: every vertex is referenced by a face and every face index is valid.
 *   Vertex order: owner node in linear order (x slowest, z fastest), then axis x, y, z.  Position, in INDEX units (no spacing, no
 *     origin): the owner's index as float, plus t = (level - v0) / (v1 - v0) on the edge's axis, v0 the owner's value: two float32
 *     subtractions, one IEEE division, one addition.
 *   Face order: cells in linear order over the (Nx - 1, Ny - 1, Nz - 1) cell grid, then table order; a face's three indices are the
 *     vertices of its three edges, normals towards increasing value.
 * nr3d_marching_cubes_count: scratch >= nr3d_marching_cubes_scratch_bytes(Nx, Ny, Nz) bytes, 8-byte aligned (48 bytes per z-row for the
 *   counts and their scans, 4 bytes per node for emit's vertex words); totals int64 [2] = {V, F}, stored with system scope (pinned host
 *   memory + nr3d_wait_host_words, or device memory).
 * nr3d_marching_cubes_emit: the same volume, level and scratch, V and F as read back; verts float32 [V, 3] and faces int64 [F, 3], both
 *   fully written, no row >= V / F is ever written.  V < 2^29; V == 0 is a no-op.
 * One wave per z-row, lane = z in chunks of 64 with two halo lanes; ranks from ballots and popcounts; no LDS, no atomics. */
uint64_t nr3d_marching_cubes_scratch_bytes(uint32_t Nx, uint32_t Ny, uint32_t Nz);
int nr3d_marching_cubes_count(const float *volume, uint32_t Nx, uint32_t Ny, uint32_t Nz, float level, void *scratch, int64_t *totals,
                              void *stream);
int nr3d_marching_cubes_emit(const float *volume, uint32_t Nx, uint32_t Ny, uint32_t Nz, float level, void *scratch, uint64_t V, uint64_t F,
                             float *verts, int64_t *faces, void *stream);

/* ---- k nearest neighbours between two batched point clouds (csrc/knn.hip; the reference's externals/pytorch3d_knn behind
 * nr3d_lib/maths/pytorch3d_knn.py and maths/chamfer_distance.py).  Brute force, as there; no spatial index.  An addition that touches no
 * existing entry: the ABI number stays.
 *   p1 float32 [N, P1, D], p2 float32 [N, P2, D], contiguous.  lengths1 / lengths2: int64 [N] ON THE DEVICE (the kernels read them: no
 *     host read-back), NULL = every cloud has full length; a value outside [0, P] is clamped into it.
 *   Distance of a pair, all in float32, d_c = p1[c] - p2[c]:
 *     norm == 2: dist = d_0 * d_0, then dist = fmaf(d_c, d_c, dist) for c = 1 .. D-1 (the order of the reference's loop, knn.cu:56-62,
 *                under nvcc's default contraction; this library is built without contraction, so the fmaf is written out);
 *     norm == 1: dist = |d_0|, then dist = dist + |d_c|.
 *   Row (n, i) with i < lengths1[n]: the k = min(K, lengths2[n]) smallest pairs (dist, j) in LEXICOGRAPHIC order over j < lengths2[n]:
 *     ascending distance, equal distances by ascending j, and at the K-th place the lower index wins (one of the outcomes the reference
 *     can produce: its MinK::add replaces on a strict < only).  The order is fixed: the same bytes run after run.  Slots k .. K-1 hold
 *     dists = 0, idx = 0.  Rows i >= lengths1[n] are all zero.  Every element of dists float32 [N, P1, K] and idx int64 [N, P1, K] is
 *     written: they may be allocated uninitialised.
 *   The output is ALWAYS sorted (the reference's return_sorted=False would return the same set in an unspecified order), and there is
 *     one implementation per (D, K): the reference's `version` has nothing to select.
 *   Non-finite coordinates or distances: the neighbours of an affected row (a non-finite p1 row; every row of a cloud whose p2 holds
 *     a non-finite point; a row with a pair of finite points so far apart that its float32 distance overflows to +inf: such a pair
 *     never enters a list, since inf < inf is false, so the row can come back with (inf, 0) entries) are unspecified, but every idx
 *     stays in [0, max(lengths2[n], 1)), no other row changes and nothing is written outside the row.
 *   Refused with a message: P1 or P2 >= 2^31, N >= 2^31, K == 0, D == 0, norm outside {1, 2}.  N == 0, P1 == 0 or P2 == 0 is a no-op
 *     (with P2 == 0 NOTHING is written: the caller returns zeros).
 *   nr3d_knn_fast_path(D, K): 1 when k_knn<D, KB, NORM> serves the pair (D in 1..8, K <= 32 in buckets KB = 1, 4, 8, 16, 32: a lane owns
 *     1, 2 or 4 queries in registers, p2 streams through LDS in tiles of nr3d_knn_tile_points(D) points read as broadcasts, the top-K is
 *     a sorted list in statically indexed registers); 0: k_knn_any, one lane per query, p2 from global memory, the list in the row's
 *     own output slots -- the same contract, CORRECT AND UNOPTIMISED.
 *   nr3d_knn_tile_points(D): the tile length of the fast kernel for this D, 0 without one (tests place P2 around it).
 *   nr3d_knn_launch_plan(N, P1, D, K): what nr3d_knn_points launches for N clouds of P1 query points: 0 when k_knn_any serves (D, K),
 *     else R | wg << 8, R = query points per lane (1, 2 or 4), wg = lanes per workgroup (64, 128 or 256); a workgroup covers wg R
 *     consecutive rows of one cloud.  Computed by the function the launcher itself calls, no device is touched (tests assert the
 *     variant they mean to run before they run it).  An addition that touches no existing entry: the ABI number stays.
 * nr3d_knn_points_backward: idx int64 [N, P1, K] and grad_dists float32 [N, P1, K] as the forward shaped them.  For k < min(K,
 *   lengths2[n]), i < lengths1[n] and each c:  norm == 2: t = 2 g[n,i,k] (p1 - p2[idx]);  norm == 1: t = g (p1 > p2 ? 1 : -1) (at
 *   equality -1 for p1, as in the reference).  grad_p1 float32 [N, P1, D]: the lane's own sum over k, fully written without atomics
 *   (deterministic; rows >= lengths1[n] zero).  grad_p2 float32 [N, P2, D], zero-init: takes -t through float32 atomic adds.  An idx
 *   outside [0, P2) is skipped.  N == 0, P1 == 0 or P2 == 0 is a no-op.  No double backward (the reference is once_differentiable). */
int nr3d_knn_points(const float *p1, const float *p2, const int64_t *lengths1, const int64_t *lengths2, uint64_t N, uint64_t P1, uint64_t P2,
                    uint32_t D, uint32_t K, int norm, float *dists, int64_t *idx, void *stream);
int nr3d_knn_points_backward(const float *p1, const float *p2, const int64_t *lengths1, const int64_t *lengths2, const int64_t *idx,
                             const float *grad_dists, uint64_t N, uint64_t P1, uint64_t P2, uint32_t D, uint32_t K, int norm, float *grad_p1,
                             float *grad_p2, void *stream);
int nr3d_knn_fast_path(uint32_t D, uint32_t K);
int nr3d_knn_tile_points(uint32_t D);
int nr3d_knn_launch_plan(uint64_t N, uint64_t P1, uint32_t D, uint32_t K);

/* ---- ray test of a forest of blocks (csrc/forest_ray_test.hip; ForestBlockSpace.ray_test, nr3d_lib/models/spatial/forest.py:353-394,
 * which tests every ray against every block box because the octree traversal it wanted, :302-351, stood on kaolin's SPC ray trace).
 * One descent of the forest's byte octree per ray, pruning whole subtrees; the result is the dense route's, BIT FOR BIT.  An addition
 * that touches no existing entry: the ABI number stays.
 *   forest: octree / exsum as above (both may be NULL on level 0: the root is the only block), level <= 15, world_block_size > 0;
 *     block_ks is NOT read: a block's coordinates are those of its path through the octree, which is what block_ks holds.
 *   rays_o, rays_d float32 [R, 3]; near / far: float32 [R] per ray, or NULL and then near_const / far_const for every ray
 *     (no lower bound: NULL, 0; no upper bound: NULL, +inf -- min(x, +inf) is x, and a NaN stays one).  wb = world_block_size,
 *     wo = world_origin; all in float32, no contraction:
 *   Block k:   bmin = float(k) * wb + wo,  bmax = bmin + wb            (an explicit multiply, then an add)
 *   Per axis:  t0 = (bmin - o) / d,  t1 = (bmax - o) / d               (IEEE subtraction and division: x / 0 = +-inf, 0 / 0 = NaN)
 *   entry = max(max over the axes of min(t0, t1), near),  exit = min(min over the axes of max(t0, t1), far), where min and max
 *     PROPAGATE NaN (torch.minimum / torch.maximum; fminf / fmaxf would not).  A ray parallel to a slab with its origin exactly on one
 *     of the slab's planes gives 0 / 0: that pair is rejected, as by the dense route.
 *   Hit:       exit > entry && exit > 0.
 *   Order:     the segments of a ray by (entry, block index) ascending -- a stable sort by entry of the hits in block order; block
 *     index = node index - level_poffset.  The order is fixed: the same bytes run after run.
 *   Interior nodes (why no hit is lost, without an epsilon): node k on level l of L is tested on lo = float(k 2^(L-l)) * wb + wo and
 *     hi = (float((k + 1) 2^(L-l) - 1) * wb + wo) + wb, the planes of its first and last leaf by the expression above.  int -> float,
 *     * wb (> 0), + wo, - o and / d for a fixed d != 0 are monotone under round-to-nearest, so every leaf's float interval lies inside
 *     its ancestors' and the non-strict test exit >= entry && exit >= 0 is conservative; with d == 0 on an axis a node accepts
 *     lo <= o <= hi, the leaf keeps the NaN / inf arithmetic.  Children are visited front to back (c ^ sign mask of d).
 *   _count: counts int64 [R] = segments per ray, fully written.  Then nr3d_prune_compact_packs(R, counts, ...) gives begin_all, the hit
 *     rays, their pack_infos and the totals {S, hit rays}: the one device->host wait.
 *   _emit: seg_block_inds int64 [S], seg_entries / seg_exits float32 [S], fully written (the packs tile [0, S)); a ray whose
 *     begin_all + counts leaves [0, S] writes nothing.
 *   Refused with a message: level > 15, n_trees == 0, R >= 2^28 (nr3d_prune_compact_packs), a world_block_size that is not positive,
 *     S > R * n_trees.  R == 0 (and S == 0 for _emit) is a no-op. */
int nr3d_forest_ray_test_count(const nr3d_forest_meta_t *forest, uint32_t n_rays, const float *rays_o, const float *rays_d,
                               const float *near, float near_const, const float *far, float far_const, int64_t *counts, void *stream);
int nr3d_forest_ray_test_emit(const nr3d_forest_meta_t *forest, uint32_t n_rays, const float *rays_o, const float *rays_d,
                              const float *near, float near_const, const float *far, float far_const, const int64_t *counts,
                              const int64_t *begin_all, uint64_t S, int64_t *seg_block_inds, float *seg_entries, float *seg_exits,
                              void *stream);

/* ---- pixel importance sampling on accumulated error maps (csrc/importance.hip; ErrorMap / ImpSampler of
 * nr3d_lib/models/importance.py, which runs every step below as a chain of torch ops).  Additions that touch no existing entry: the ABI
 * number stays.  All arithmetic is float32 with one rounding per operation (no contraction, IEEE division), in the order written here.
 *
 * _sample: one launch, one lane per sample s of n_samples.  u_img, u_x, u_y float32 [n_samples] (the caller clamps them to
 *   [1e-6, 1 - 1e-6]); u_img is read for sampled frames only.  lower(row, len, u) = min(the first k with row[k] >= u, len - 1):
 *   searchsorted(right=False) with a clamp that no valid CDF reaches and that keeps every read inside its row.
 *     s <  n_uniform:  i = min(int(u_img * float(n_images)), n_images - 1),  xy = (u_x, u_y)
 *     s >= n_uniform:  the map is the last of maps[0 .. n_maps) with first <= s (maps[0].first == n_uniform, firsts non-decreasing:
 *       a map whose segment is empty shares its first with the next one);
 *       i = lower(cdf_img, n_images, u_img);  h = lower(cdf_y[i], res_y, u_y);  prev = h > 0 ? cdf_y[i, h-1] : 0;
 *       y = ((u_y - prev) / (cdf_y[i, h] - prev) + float(h)) / float(res_y);  w, x the same way from cdf_x_cond_y[i, h] and u_x.
 *   frame_mode: _SAMPLED as above; _CONST: i = frame_const for every sample; _TENSOR: i = frame_ind[s] (int64 [n_samples]); negative
 *     frames count from the end as torch's do, then clamp to [0, n_images).
 *   out_i int64 [n_samples], out_xy float32 [n_samples, 2] (x first): either may be NULL and is then not computed; fully written.
 *   maps: a HOST array of n_maps <= NR3D_IMPORTANCE_MAX_MAPS entries (copied into the launch), all maps with n_images images.
 *
 * _update: error_map float32 [n_images, res_y, res_x] += the bilinear splat of val float32 [n] at xy float32 [n, 2] of frame frame_ind[s]
 *   (int64 [n]) or, frame_ind NULL, frame_const.  Per sample: wf = x * float(res_x), w = trunc(wf), w_w = wf - float(w), THEN w is
 *   clamped to [0, res_x - 2]; the same in y; contributions ((1-w_h)(1-w_w)) val -> (h, w), (w_h (1-w_w)) val -> (h+1, w),
 *   ((1-w_h) w_w) val -> (h, w+1), (w_h w_w) val -> (h+1, w+1).  Each contribution c, clamped to |c| <= 2^16, is added as
 *   llrint(double(c) * 2^32) to acc (int64 [n_images, res_y, res_x], ALL ZERO on entry) with a 64-bit integer atomic; a second launch
 *   takes every touched cell out of acc with an exchange against 0 and adds float(double(sum) * 2^-32) to the map's cell, one writer
 *   per cell.  acc is all zero again on return; the map's bytes do not depend on the order of arrival.  Dropped without any write: a
 *   frame outside [0, n_images), a non-finite x, y, val or product with the resolution, val < 0.
 *   Refused: n > NR3D_IMPORTANCE_UPDATE_CHUNK (the caller splits), res_y < 2 or res_x < 2.
 *
 * _construct_cdf: three launches, no atomics.  scan(v [L]): 64-element chunks in order; inside a chunk the Kogge-Stone inclusive scan
 *   (steps 1, 2, ... 32: v[j] += v[j - step] for j >= step, all j at once), then the carry -- the previous chunk's last result, 0.0f
 *   before the first -- is added to every element of the chunk.  total = the result at the row's LAST ELEMENT (so norm()'s last value is a, not a ratio of two trees).
 *   norm(c [L], total) [k] = (a * c[k]) / total + b * (float(k + 1) / float(L)),  a = one_minus_min_pdf, b = min_pdf.
 *     e = error_map[n, h, :], clamped from above to max_pdf when has_max_pdf (the clamped value is stored back; with `clean` 0 is);
 *     c = scan(e + 1e-10f): cdf_x_cond_y[n, h] = norm(c, total), pdf_y[n, h] = total;
 *     cdf_y[n] = norm(scan(pdf_y[n]), total), pdf_img[n] = total;  cdf_img = norm(scan(pdf_img), total).
 *   pdf_y float32 [n_images, res_y] and pdf_img float32 [n_images] are the caller's workspace; all outputs fully written. */
#define NR3D_IMPORTANCE_MAX_MAPS 8
#define NR3D_IMPORTANCE_UPDATE_CHUNK 32768
#define NR3D_IMPORTANCE_FRAME_SAMPLED 0
#define NR3D_IMPORTANCE_FRAME_CONST 1
#define NR3D_IMPORTANCE_FRAME_TENSOR 2
typedef struct nr3d_importance_map {
	const float *cdf_img;         /* [n_images] */
	const float *cdf_y;           /* [n_images, res_y] */
	const float *cdf_x_cond_y;    /* [n_images, res_y, res_x] */
	uint32_t res_y;
	uint32_t res_x;
	uint32_t first;               /* the first sample of this map's segment */
	uint32_t reserved;
} nr3d_importance_map_t;
int nr3d_importance_sample(uint32_t n_samples, uint32_t n_images, uint32_t n_uniform, int n_maps, const nr3d_importance_map_t *maps,
                           const float *u_img, const float *u_x, const float *u_y, int frame_mode, int64_t frame_const,
                           const int64_t *frame_ind, int64_t *out_i, float *out_xy, void *stream);
int nr3d_importance_update(uint32_t n_samples, uint32_t n_images, uint32_t res_y, uint32_t res_x, int64_t frame_const,
                           const int64_t *frame_ind, const float *xy, const float *val, float *error_map, int64_t *acc, void *stream);
int nr3d_importance_construct_cdf(uint32_t n_images, uint32_t res_y, uint32_t res_x, float *error_map, float one_minus_min_pdf,
                                  float min_pdf, int has_max_pdf, float max_pdf, int clean, float *cdf_x_cond_y, float *cdf_y,
                                  float *cdf_img, float *pdf_y, float *pdf_img, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NR3D_HIP_H */
