// nr3d_lib_amd/csrc/forest_ray_test.hip -- the ray test of a forest of blocks (nr3d_forest_ray_test_count / _emit): the (block, entry,
// exit) segments of every ray through the occupied blocks, found by ONE descent of the block octree per ray instead of a slab test on
// every (ray, block) pair, behind nr3d_lib_amd/bindings/_forest.py (forest_ray_test) and ForestBlockSpace.ray_test.
//
// The reference wanted this traversal (nr3d_lib/models/spatial/forest.py:302-351 keeps one in a string: kaolin's SPC ray trace "is very
// buggy right now") and fell back to ray-against-every-box (:353-394), a dense [R, B] chain with two nonzero() calls.  Here:
//   count: eight lanes = one ray, one per child of the ray's current node; depth-first descent of the byte octree, children front to
//          back (c ^ sign mask of d); a subtree whose box the ray misses is skipped whole; hits are counted -> counts[ray];
//   (host: nr3d_prune_compact_packs turns counts into begin_all, the hit rays, their pack_infos and the totals -- one readback)
//   emit:  the same descent writes the segments at begin_all[ray] + running count, then an insertion pass over the ray's own pack puts
//          them in (entry, block index) order (front-to-back traversal leaves them nearly sorted).
// Both kernels run the same code (template flag), compiled without contraction or fast math (Makefile), so they agree on every hit.
//
// Contract (include/nr3d_hip.h has the table): the LEAF test is the dense route's arithmetic bit for bit -- bmin = float(k) * wb + wo,
// bmax = bmin + wb, t = (plane - o) / d in IEEE float32, min / max that PROPAGATE NaN as torch.minimum / maximum do (fminf / fmaxf would
// drop it), hit = exit > entry && exit > 0.  An INTERIOR node is tested on the planes of its first and last leaf computed by the same
// expression; every operation involved (int -> float, * wb with wb > 0, + wo, - o, / d for a fixed d != 0) is monotone under
// round-to-nearest, so a leaf's float interval lies inside its ancestors' and the non-strict node test (exit >= entry && exit >= 0)
// never loses a leaf hit: no epsilon.  d == 0 on an axis is handled by hand at a node (lo <= o <= hi); the leaf keeps the 0 / 0 = NaN
// and x / 0 = inf arithmetic, which rejects a ray that lies in one of the slab's planes, as the dense route does.
//
// The per-level state of the descent is the node index of every ancestor and the mask of its children still to visit: LDS laid out
// [level][lane] (no per-lane array indexed at run time, no scratch); a node's byte and exsum are reloaded on the way back up.  A forest
// of up to kLdsNodes non-leaf nodes is walked out of an LDS copy of its bytes and exsum (k_ray_test's LDS_TREE); emit skips the
// insertion pass of a ray whose segments arrived in order.  (One lane per ray with a loop over the children was measured first: the
// chain of node tests per ray, not memory, set its time, and it lost to the dense route on deep or wide forests at 4096 rays:
// profiles/forest_ray_test_resources.txt.)
#include "common.h"

namespace nr3d {
namespace frt {

constexpr int kBlock = 128;
constexpr uint32_t kLanes = 8;           // lanes per ray: one per child of a node
constexpr uint32_t kRays = kBlock / kLanes;
constexpr int kMaxLevel = 15;            // block_ks is int16
constexpr uint32_t kLdsNodes = 8192;     // non-leaf nodes a workgroup keeps in LDS: 5 bytes each next to the 7.5 KiB of ancestors

struct Params {
	const uint8_t *octree;
	const int32_t *exsum;
	uint32_t R, level, level_poffset, n_trees;
	float wb[3], wo[3];
	const float *rays_o, *rays_d, *near, *far;
	float near_c, far_c;
};

struct Ray { float o[3], d[3], near, far; };

__device__ __forceinline__ float nan_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a < b ? a : b)); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

// the dense route's slab test on block k: (entry, exit), true for a hit
__device__ __forceinline__ bool leaf_test(const Params &p, const Ray &q, const int (&k)[3], float &entry, float &exit_) {
	float t_near = 0.0f, t_far = 0.0f;
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		const float bmin = (float)k[a] * p.wb[a] + p.wo[a];
		const float bmax = bmin + p.wb[a];
		const float t0 = (bmin - q.o[a]) / q.d[a];
		const float t1 = (bmax - q.o[a]) / q.d[a];
		const float lo = nan_min(t0, t1), hi = nan_max(t0, t1);
		t_near = a == 0 ? lo : nan_max(t_near, lo);
		t_far = a == 0 ? hi : nan_min(t_far, hi);
	}
	entry = nan_max(t_near, q.near);
	exit_ = nan_min(t_far, q.far);
	return (exit_ > entry) && (exit_ > 0.0f);
}

// conservative test of the node k on the level whose cells are 2^shift blocks wide: false only if no leaf below it can be a hit
__device__ __forceinline__ bool node_test(const Params &p, const Ray &q, const int (&k)[3], uint32_t shift) {
	float entry = q.near, exit_ = q.far;
	bool ok = true;
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		const int k0 = k[a] << shift, k1 = ((k[a] + 1) << shift) - 1;       // first and last leaf along the axis
		const float lo = (float)k0 * p.wb[a] + p.wo[a];
		const float hi = ((float)k1 * p.wb[a] + p.wo[a]) + p.wb[a];
		if (q.d[a] == 0.0f) {
			ok = ok && (lo <= q.o[a]) && (q.o[a] <= hi);
		} else {
			const float t0 = (lo - q.o[a]) / q.d[a];
			const float t1 = (hi - q.o[a]) / q.d[a];
			entry = nan_max(entry, nan_min(t0, t1));
			exit_ = nan_min(exit_, nan_max(t0, t1));
		}
	}
	return ok && (exit_ >= entry) && (exit_ >= 0.0f);                       // a NaN anywhere rejects: the leaves would hold it too
}

// 8-bit child mask (bit = child index) -> traversal order (bit i = child i ^ sm): an xor of the index swaps halves, pairs and neighbours
__device__ __forceinline__ uint32_t by_order(uint32_t m, uint32_t sm) {
	if (sm & 4u) m = ((m & 0x0Fu) << 4) | ((m & 0xF0u) >> 4);
	if (sm & 2u) m = ((m & 0x33u) << 2) | ((m & 0xCCu) >> 2);
	if (sm & 1u) m = ((m & 0x55u) << 1) | ((m & 0xAAu) >> 1);
	return m;
}

// EIGHT lanes = one ray, lane c tests child c of the ray's current node: the walk is a chain of node tests (six IEEE divisions each)
// whose latency, not the machine's throughput, is what a launch takes, and the eight children of a node are independent.  A ballot
// gathers the children that pass; the group keeps them as a pending mask per level and descends front to back.  The state of a group
// is the same in its eight lanes (every lane computes it from the same ballots), so nothing but the ballot, and in emit four
// shuffles for the order check, crosses lanes; all lanes of a wave stay in the loop until its last ray is done (the ballots need them).
// LDS_TREE: the workgroup first copies the bytes and the exsum of the non-leaf nodes (level_poffset of them) into LDS; forests above
// kLdsNodes non-leaf nodes read them from global memory.
template <bool EMIT, bool LDS_TREE>
__global__ __launch_bounds__(kBlock) void k_ray_test(Params p, int64_t *__restrict__ counts_out, const int64_t *__restrict__ counts_in,
                                                      const int64_t *__restrict__ begin_all, uint64_t S, int64_t *__restrict__ seg_b,
                                                      float *__restrict__ seg_e, float *__restrict__ seg_x) {
	extern __shared__ uint32_t smem[];
	uint32_t (*s_ord)[kBlock] = (uint32_t (*)[kBlock])smem;                       // [level][lane]: node index of the ancestor ...
	uint8_t (*s_pend)[kBlock] = (uint8_t (*)[kBlock])(smem + kMaxLevel * kBlock);  // ... and its children still to visit
	int32_t *l_exsum = (int32_t *)(smem + kMaxLevel * kBlock + kMaxLevel * kBlock / 4);
	uint8_t *l_octree = (uint8_t *)(l_exsum + p.level_poffset);
	const uint32_t lane = threadIdx.x;
	if (LDS_TREE) {
		for (uint32_t i = lane; i < p.level_poffset; i += kBlock) {
			l_exsum[i] = p.exsum[i];
			l_octree[i] = p.octree[i];
		}
		__syncthreads();
	}
	auto byte_of = [&](int32_t node) -> uint32_t { return LDS_TREE ? (uint32_t)l_octree[node] : (uint32_t)p.octree[node]; };
	auto exsum_of = [&](int32_t node) -> int32_t { return LDS_TREE ? l_exsum[node] : p.exsum[node]; };
	const uint32_t c = lane & (kLanes - 1u);                 // this lane's child
	const uint32_t gbase = lane & 63u & ~(kLanes - 1u);      // the group's first lane in its wave
	const uint32_t ray = blockIdx.x * kRays + lane / kLanes;
	const bool valid = ray < p.R;
	bool active = valid;                                     // no lane leaves before the loop ends
	uint64_t base = 0, cap = 0;
	if (EMIT && valid) {
		const int64_t cn = counts_in[ray], b = begin_all[ray];
		if (cn <= 0 || b < 0 || (uint64_t)b + (uint64_t)cn > S) active = false;      // nothing to write, or counts that are not this call's
		else {
			base = (uint64_t)b;
			cap = (uint64_t)cn;
		}
	}
	Ray q;
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		q.o[a] = valid ? p.rays_o[3 * (size_t)ray + a] : 0.0f;
		q.d[a] = valid ? p.rays_d[3 * (size_t)ray + a] : 0.0f;
	}
	q.near = (valid && p.near) ? p.near[ray] : p.near_c;
	q.far = (valid && p.far) ? p.far[ray] : p.far_c;

	const uint32_t L = p.level;
	uint64_t n = 0;
	bool in_order = true;                                    // emit: every segment so far came at or behind the one before it
	int k[3] = {0, 0, 0};
	if (L == 0) {                                            // the root is the only block (uniform over the launch)
		float e, x;
		if (active && c == 0u && leaf_test(p, q, k, e, x)) {
			if (EMIT) {
				seg_b[base] = 0;
				seg_e[base] = e;
				seg_x[base] = x;
			}
			n = 1;
		}
		if (!EMIT && valid && c == 0u) counts_out[ray] = (int64_t)n;
		return;
	}
	active = active && node_test(p, q, k, L);
	const uint32_t sm = (q.d[0] < 0.0f ? 4u : 0u) | (q.d[1] < 0.0f ? 2u : 0u) | (q.d[2] < 0.0f ? 1u : 0u);
	const uint32_t i = c ^ sm;                               // this lane's place in the front-to-back order
	uint32_t depth = 0, pend = 0;
	int32_t ord = 0, first = 0, last_b = 0;
	uint32_t bits = 0;
	float last_e = 0.0f;
	if (active) {
		bits = byte_of(0);
		first = exsum_of(0);                                 // the node before the first child
	}
	while (__ballot(active) != 0ull) {
		// the children of the group's node (ord, k, depth): blocks when the node is on level L - 1
		const bool leaf_level = depth + 1u == L;
		const bool exists = active && ((bits >> c) & 1u);
		const int32_t child = first + (int32_t)__popc(bits & ((2u << c) - 1u));           // as identify(): inclusive count
		const int32_t bidx = child - (int32_t)p.level_poffset;
		const int ck[3] = {(k[0] << 1) | (int)((c >> 2) & 1u), (k[1] << 1) | (int)((c >> 1) & 1u), (k[2] << 1) | (int)(c & 1u)};
		bool pass = false;
		float e = 0.0f, x = 0.0f;
		if (exists) {
			if (leaf_level) pass = bidx >= 0 && (uint32_t)bidx < p.n_trees && leaf_test(p, q, ck, e, x);
			else pass = node_test(p, q, ck, L - depth - 1u);
		}
		const uint32_t ordered = by_order((uint32_t)(__ballot(pass) >> gbase) & 0xFFu, sm);
		const uint32_t before = ordered & ((1u << i) - 1u);  // the passing children in front of this lane's
		if (EMIT) {
			if (__ballot(active && leaf_level) != 0ull) {    // wave-uniform: the shuffles below run in every lane
				// a segment against the one written before it: of this node, or the last of the node before
				const uint32_t ip = before ? 31u - (uint32_t)__clz(before) : i;
				const float pe = __shfl(e, (int)(gbase + (ip ^ sm)));
				const int32_t pb = __shfl(bidx, (int)(gbase + (ip ^ sm)));
				const float qe = before ? pe : last_e;
				const int32_t qb = before ? pb : last_b;
				const bool late = pass && leaf_level && (before != 0u || n > 0) && (qe > e || (qe == e && qb > bidx));
				if (((uint32_t)(__ballot(late) >> gbase) & 0xFFu) != 0u) in_order = false;
				const uint32_t il = ordered ? 31u - (uint32_t)__clz(ordered) : i;
				const float le = __shfl(e, (int)(gbase + (il ^ sm)));
				const int32_t lb = __shfl(bidx, (int)(gbase + (il ^ sm)));
				if (active && leaf_level && ordered != 0u) {
					last_e = le;
					last_b = lb;
				}
			}
		}
		if (active) {
			if (leaf_level) {
				if (EMIT && pass) {
					const uint64_t at = n + (uint64_t)__popc(before);
					if (at < cap) {
						seg_b[base + at] = (int64_t)bidx;
						seg_e[base + at] = e;
						seg_x[base + at] = x;
					}
				}
				n += (uint64_t)__popc(ordered);
				pend = 0;
			} else {
				pend = ordered;
			}
			// on to the next node: back up while nothing is pending, then down into the first pending child
			while (pend == 0u) {
				if (depth == 0u) {
					active = false;
					break;
				}
				--depth;
#pragma unroll
				for (int a = 0; a < 3; ++a) k[a] >>= 1;
				ord = (int32_t)s_ord[depth][lane];
				pend = s_pend[depth][lane];
				bits = byte_of(ord);
				first = exsum_of(ord);
			}
			if (active) {
				const uint32_t cc = ((uint32_t)__ffs((int)pend) - 1u) ^ sm;
				pend &= pend - 1u;
				s_ord[depth][lane] = (uint32_t)ord;
				s_pend[depth][lane] = (uint8_t)pend;
				++depth;
				ord = first + (int32_t)__popc(bits & ((2u << cc) - 1u));
				k[0] = (k[0] << 1) | (int)((cc >> 2) & 1u);
				k[1] = (k[1] << 1) | (int)((cc >> 1) & 1u);
				k[2] = (k[2] << 1) | (int)(cc & 1u);
				bits = byte_of(ord);
				first = exsum_of(ord);
				pend = 0;
			}
		}
	}
	if (!EMIT) {
		if (valid && c == 0u) counts_out[ray] = (int64_t)n;
		return;
	}
	// (entry, block) ascending over the ray's own pack: one lane reads back what the group wrote (the kernel's end orders the stores of a
	// wave's lanes no more than program order does: fence first)
	if (in_order || c != 0u || cap == 0) return;
	__threadfence();
	const uint64_t m = n < cap ? n : cap;
	for (uint64_t s = 1; s < m; ++s) {
		const float e = seg_e[base + s], x = seg_x[base + s];
		const int64_t b = seg_b[base + s];
		uint64_t j = s;
		while (j > 0) {
			const float ep = seg_e[base + j - 1];
			const int64_t bp = seg_b[base + j - 1];
			if (!(ep > e || (ep == e && bp > b))) break;
			seg_e[base + j] = ep;
			seg_b[base + j] = bp;
			seg_x[base + j] = seg_x[base + j - 1];
			--j;
		}
		if (j != s) {
			seg_e[base + j] = e;
			seg_b[base + j] = b;
			seg_x[base + j] = x;
		}
	}
}

static int make_params(const char *fn, const nr3d_forest_meta_t *fo, uint32_t R, const float *rays_o, const float *rays_d, const float *near,
                       float near_const, const float *far, float far_const, Params &p) {
	NR3D_CHECK(fo, "%s: forest meta is NULL", fn);
	NR3D_CHECK(fo->level <= (uint32_t)kMaxLevel, "%s: level = %u, at most %d (block_ks is int16)", fn, fo->level, kMaxLevel);
	NR3D_CHECK(fo->n_trees >= 1, "%s: a forest without blocks", fn);
	NR3D_CHECK(fo->level == 0 || (fo->octree && fo->exsum), "%s: NULL octree / exsum on level %u", fn, fo->level);
	NR3D_CHECK(R < (1u << 28), "%s: R = %u rays, fewer than 2^28 per call", fn, R);
	NR3D_CHECK(R == 0 || (rays_o && rays_d), "%s: NULL rays_o / rays_d", fn);
	for (int a = 0; a < 3; ++a)
		NR3D_CHECK(fo->world_block_size[a] > 0.0f, "%s: world_block_size[%d] = %g, must be positive", fn, a, (double)fo->world_block_size[a]);
	p.octree = fo->octree;
	p.exsum = fo->exsum;
	p.R = R;
	p.level = fo->level;
	p.level_poffset = fo->level_poffset;
	p.n_trees = fo->n_trees;
	for (int a = 0; a < 3; ++a) {
		p.wb[a] = fo->world_block_size[a];
		p.wo[a] = fo->world_origin[a];
	}
	p.rays_o = rays_o;
	p.rays_d = rays_d;
	p.near = near;
	p.far = far;
	p.near_c = near_const;
	p.far_c = far_const;
	return 0;
}

static inline bool lds_tree(const Params &p) { return p.level > 0 && p.level_poffset <= kLdsNodes; }
static inline uint32_t lds_bytes(const Params &p) {
	return (uint32_t)(kMaxLevel * kBlock * (sizeof(uint32_t) + 1)) + (lds_tree(p) ? ((p.level_poffset * 5u + 3u) & ~3u) : 0u);
}

}  // namespace frt
}  // namespace nr3d

using namespace nr3d;

extern "C" int nr3d_forest_ray_test_count(const nr3d_forest_meta_t *forest, uint32_t n_rays, const float *rays_o, const float *rays_d,
                                          const float *near, float near_const, const float *far, float far_const, int64_t *counts,
                                          void *stream) {
	frt::Params p;
	NR3D_TRY(frt::make_params("forest_ray_test_count", forest, n_rays, rays_o, rays_d, near, near_const, far, far_const, p));
	if (n_rays == 0) return 0;
	NR3D_CHECK(counts, "forest_ray_test_count: NULL counts");
	const auto kernel = frt::lds_tree(p) ? frt::k_ray_test<false, true> : frt::k_ray_test<false, false>;
	hipLaunchKernelGGL(kernel, dim3(div_up(n_rays, frt::kRays)), dim3(frt::kBlock), frt::lds_bytes(p), (hipStream_t)stream, p, counts, (const int64_t *)nullptr,
	                   (const int64_t *)nullptr, (uint64_t)0, (int64_t *)nullptr, (float *)nullptr, (float *)nullptr);
	NR3D_LAUNCH_CHECK();
	return 0;
}

extern "C" int nr3d_forest_ray_test_emit(const nr3d_forest_meta_t *forest, uint32_t n_rays, const float *rays_o, const float *rays_d,
                                         const float *near, float near_const, const float *far, float far_const, const int64_t *counts,
                                         const int64_t *begin_all, uint64_t S, int64_t *seg_block_inds, float *seg_entries,
                                         float *seg_exits, void *stream) {
	frt::Params p;
	NR3D_TRY(frt::make_params("forest_ray_test_emit", forest, n_rays, rays_o, rays_d, near, near_const, far, far_const, p));
	if (n_rays == 0 || S == 0) return 0;
	NR3D_CHECK(counts && begin_all, "forest_ray_test_emit: NULL counts / begin_all");
	NR3D_CHECK(seg_block_inds && seg_entries && seg_exits, "forest_ray_test_emit: NULL seg_block_inds / seg_entries / seg_exits");
	NR3D_CHECK(S <= (uint64_t)n_rays * forest->n_trees, "forest_ray_test_emit: S = %llu segments from %u rays x %u blocks",
	           (unsigned long long)S, n_rays, forest->n_trees);
	const auto kernel = frt::lds_tree(p) ? frt::k_ray_test<true, true> : frt::k_ray_test<true, false>;
	hipLaunchKernelGGL(kernel, dim3(div_up(n_rays, frt::kRays)), dim3(frt::kBlock), frt::lds_bytes(p), (hipStream_t)stream, p, (int64_t *)nullptr, counts, begin_all, S, seg_block_inds,
	                   seg_entries, seg_exits);
	NR3D_LAUNCH_CHECK();
	return 0;
}
