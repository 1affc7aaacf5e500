// nr3d_lib_amd/csrc/marching_cubes.hip -- marching cubes on a float32 volume that never leaves the device (nr3d_marching_cubes_count /
// _emit): one vertex per live edge, the triangles of the generated case table (mc_table.inc, tools/gen_mc_table.py), both in a canonical
// order, so that the result is the same bytes run after run and equals the numpy restatement (tests/marching_cubes_ref.py) bit for bit.
//
// The reference has no kernel for this: it copies every SDF value to the host and runs skimage.measure.marching_cubes on one core
// (nr3d_lib/graphics/trianglemesh.py:210-214).  The specification is in include/nr3d_hip.h.
//
// The unit of work is one z-row of nodes: one wave per row (i, j), lane = z, four rows per workgroup.  Everything a lane has to know
// about its neighbours arrives as 64-bit ballots:
//   F[di][dj]  the finite nodes of the 3 x 3 rows around (i, j); zf = F & (F >> 1): z and z + 1 both finite
//   A[ci][cj]  the active cells of the 2 x 2 cell rows around the node row = AND of the zf of their four node rows
//   an edge is live iff it crosses the level and one of its up to four cells is active: bit tests on A and A << 1
// A chunk covers 64 consecutive z; its first and last lane are halo (the cells below the first owner, z + 1 of the last one), so a
// chunk advances by 62 owners.  The re-reads of the 3 x 3 neighbourhood are cache hits (a row is read by its nine neighbours at about the
// same time); no LDS, no atomics.
//   count:  per row, the live edges its nodes own and the triangles of its cell row (ranks inside a chunk: popcounts of ballots)
//           -> two exclusive scans over the rows (scan.h), the totals V and F into two pinned words: the ONE readback
//   emit 1: the vertices, and per node a scratch word  first vertex id << 3 | live-axis mask  (uint32: V < 2^29)
//   emit 2: the faces: a cell reads the words of the up to 7 distinct owner nodes of its edges and ranks the axis inside the mask
//           (a launch boundary separates it from emit 1: the words come from other workgroups)
// Rows that own no vertex / no triangle leave at once in the emit launches (their counts are in the scan's output).  Workgroups take
// rows in launch order: handing each XCD a contiguous range of rows was measured and is not done (it leaves count where it is and piles
// the rows that do not leave early onto a few XCDs in emit).
//
// Compiled without contraction or fast math (Makefile): t = (level - v0) / (v1 - v0) is two subtractions and one IEEE division, the
// position one addition; count and emit take every decision from the same expressions.
#include "common.h"
#include "scan.h"
#include "mc_table.inc"

namespace nr3d {
namespace mc {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kOwners = 62;         // lanes 1..62 of a node-row chunk own nodes; lane 0 and lane 63 are halo
constexpr uint32_t kCells = 63;          // lanes 0..62 of a cell-row chunk own cells; lane 63 is the z + 1 halo

__device__ __forceinline__ bool is_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool crosses(float a, float b, float level) { return ((a < level) && (b >= level)) || ((a >= level) && (b < level)); }

// the case index of the cell at this lane's z from the inside-ballots of its four node rows I[dx][dy] (corner c at (c & 1, (c >> 1) & 1,
// (c >> 2) & 1)); the lane above must be in the wave
__device__ __forceinline__ uint32_t cell_case(const uint64_t I[2][2], uint32_t lane) {
	uint32_t c = 0;
#pragma unroll
	for (int k = 0; k < 8; ++k) c |= (uint32_t)((I[k & 1][(k >> 1) & 1] >> (lane + ((k >> 2) & 1))) & 1ull) << k;
	return c;
}

// the sum over the wave of a lane value n < 8, and the sum over the lanes below
__device__ __forceinline__ uint32_t wave_sum3(uint32_t n, uint64_t below, uint32_t &before) {
	const uint64_t b0 = __ballot(n & 1u), b1 = __ballot(n & 2u), b2 = __ballot(n & 4u);
	before = (uint32_t)__popcll(b0 & below) + 2u * (uint32_t)__popcll(b1 & below) + 4u * (uint32_t)__popcll(b2 & below);
	return (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1) + 4u * (uint32_t)__popcll(b2);
}

// node rows: count (cnt_v, cnt_f) or emit (verts, words)
template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_rows(const float *__restrict__ vol, uint32_t Nx, uint32_t Ny, uint32_t Nz, float level,
                                                 int64_t *__restrict__ cnt_v, int64_t *__restrict__ cnt_f,
                                                 const int64_t *__restrict__ vinfo, uint64_t V, float *__restrict__ verts,
                                                 uint32_t *__restrict__ words) {
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t row = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
	if (row >= Nx * Ny) return;
	const uint32_t i = row / Ny, j = row % Ny;
	uint64_t vbase = 0, nf = 0;
	if (EMIT) {
		if (vinfo[2 * (size_t)row + 1] == 0) return;          // no vertex owned here: nobody reads this row's words
		vbase = (uint64_t)vinfo[2 * (size_t)row];
	}
	const uint64_t bit = 1ull << lane, below = bit - 1ull;
	const float nanv = __builtin_nanf("");
	for (uint32_t k0 = 0; k0 < Nz; k0 += kOwners) {
		const int64_t z = (int64_t)k0 - 1 + (int64_t)lane;
		const bool zin = z >= 0 && z < (int64_t)Nz;
		float v[3][3];
		uint64_t F[3][3];
#pragma unroll
		for (int di = 0; di < 3; ++di) {
#pragma unroll
			for (int dj = 0; dj < 3; ++dj) {
				const int64_t ii = (int64_t)i + di - 1, jj = (int64_t)j + dj - 1;
				const bool in = ii >= 0 && ii < (int64_t)Nx && jj >= 0 && jj < (int64_t)Ny && zin;
				v[di][dj] = in ? vol[((size_t)ii * Ny + (size_t)jj) * Nz + (size_t)z] : nanv;
				F[di][dj] = __ballot(is_finite(v[di][dj]));
				F[di][dj] &= F[di][dj] >> 1;                      // z and z + 1 finite
			}
		}
		uint64_t A[2][2];
#pragma unroll
		for (int ci = 0; ci < 2; ++ci)
#pragma unroll
			for (int cj = 0; cj < 2; ++cj) A[ci][cj] = F[ci][cj] & F[ci + 1][cj] & F[ci][cj + 1] & F[ci + 1][cj + 1];
		const float v0 = v[1][1], vx = v[2][1], vy = v[1][2], vz = __shfl_down(v0, 1, 64);
		const bool owner = lane >= 1 && lane <= kOwners && z < (int64_t)Nz;
		const uint64_t Cx = A[1][0] | A[1][1], Cy = A[0][1] | A[1][1], Cz = A[0][0] | A[0][1] | A[1][0] | A[1][1];
		const bool lx = owner && crosses(v0, vx, level) && (((Cx | (Cx << 1)) & bit) != 0);
		const bool ly = owner && crosses(v0, vy, level) && (((Cy | (Cy << 1)) & bit) != 0);
		const bool lz = owner && crosses(v0, vz, level) && ((Cz & bit) != 0);
		const uint64_t mx = __ballot(lx), my = __ballot(ly), mz = __ballot(lz);
		if (EMIT) {
			if (owner) {
				uint64_t id = vbase + (uint64_t)(__popcll(mx & below) + __popcll(my & below) + __popcll(mz & below));
				words[(size_t)row * Nz + (size_t)z] = ((uint32_t)id << 3) | (lx ? 1u : 0u) | (ly ? 2u : 0u) | (lz ? 4u : 0u);
				const float fi = (float)i, fj = (float)j, fz = (float)(uint32_t)z;
				if (lx && id < V) {
					const float t = (level - v0) / (vx - v0);
					verts[3 * id] = fi + t; verts[3 * id + 1] = fj; verts[3 * id + 2] = fz;
				}
				id += lx ? 1u : 0u;
				if (ly && id < V) {
					const float t = (level - v0) / (vy - v0);
					verts[3 * id] = fi; verts[3 * id + 1] = fj + t; verts[3 * id + 2] = fz;
				}
				id += ly ? 1u : 0u;
				if (lz && id < V) {
					const float t = (level - v0) / (vz - v0);
					verts[3 * id] = fi; verts[3 * id + 1] = fj; verts[3 * id + 2] = fz + t;
				}
			}
		} else {
			uint64_t I[2][2];
#pragma unroll
			for (int dx = 0; dx < 2; ++dx)
#pragma unroll
				for (int dy = 0; dy < 2; ++dy) I[dx][dy] = __ballot(v[1 + dx][1 + dy] < level);
			const bool active = owner && ((A[1][1] & bit) != 0);
			const uint32_t n = active ? (uint32_t)MC_NTRI[cell_case(I, lane)] : 0u;
			uint32_t before;
			nf += wave_sum3(n, below, before);
		}
		vbase += (uint64_t)(__popcll(mx) + __popcll(my) + __popcll(mz));
	}
	if (!EMIT && lane == 0) {
		cnt_v[row] = (int64_t)vbase;
		cnt_f[row] = (int64_t)nf;
	}
}

// cell rows: the faces.  Edge e = 4 a + u + 2 v of cell (i, j, k) is owned by node (i, j, k) + p0(e); its vertex is the owner's first
// id plus the live axes below a.
__global__ __launch_bounds__(kBlock) void k_faces(const float *__restrict__ vol, uint32_t Nx, uint32_t Ny, uint32_t Nz, float level,
                                                  const int64_t *__restrict__ finfo, uint64_t nF, const uint32_t *__restrict__ words,
                                                  int64_t *__restrict__ faces) {
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t row = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
	if (row >= Nx * Ny) return;
	const uint32_t i = row / Ny, j = row % Ny;
	if (i + 1 >= Nx || j + 1 >= Ny || finfo[2 * (size_t)row + 1] == 0) return;
	uint64_t fbase = (uint64_t)finfo[2 * (size_t)row];
	const uint64_t bit = 1ull << lane, below = bit - 1ull;
	for (uint32_t k0 = 0; k0 + 1 < Nz; k0 += kCells) {
		const uint32_t z = k0 + lane;
		uint64_t A = ~0ull, I[2][2];
#pragma unroll
		for (int dx = 0; dx < 2; ++dx) {
#pragma unroll
			for (int dy = 0; dy < 2; ++dy) {
				const float v = z < Nz ? vol[((size_t)(i + dx) * Ny + (size_t)(j + dy)) * Nz + z] : __builtin_nanf("");
				const uint64_t f = __ballot(is_finite(v));
				A &= f & (f >> 1);
				I[dx][dy] = __ballot(v < level);
			}
		}
		const bool active = lane < kCells && ((A & bit) != 0);
		const uint32_t cs = active ? cell_case(I, lane) : 0u;
		const uint32_t n = active ? (uint32_t)MC_NTRI[cs] : 0u;
		uint32_t before;
		const uint32_t total = wave_sum3(n, below, before);
		uint64_t f = fbase + before;
		for (uint32_t t = 0; t < n; ++t, ++f) {
			if (f >= nF) break;
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				const uint32_t e = (uint32_t)MC_TRI[cs][3 * t + c];
				const uint32_t a = e >> 2, u = e & 1u, w = (e >> 1) & 1u;
				const uint32_t dx = a == 0 ? 0u : u, dy = a == 0 ? u : (a == 1 ? 0u : w), dz = a == 2 ? 0u : w;
				const uint32_t word = words[((size_t)(i + dx) * Ny + (size_t)(j + dy)) * Nz + (size_t)(z + dz)];
				faces[3 * f + c] = (int64_t)((word >> 3) + (uint32_t)__popc(word & ((1u << a) - 1u)));
			}
		}
		fbase += total;
	}
}

struct Scratch {
	int64_t *vinfo, *finfo, *cnt_v, *cnt_f;
	void *scan_tmp;
	uint32_t *words;
	uint64_t bytes;
};

static inline uint64_t align16(uint64_t b) { return (b + 15) / 16 * 16; }

static Scratch carve(void *base, uint32_t Nx, uint32_t Ny, uint32_t Nz) {
	const uint64_t R = (uint64_t)Nx * Ny;
	char *p = (char *)base;
	Scratch s;
	uint64_t off = 0;
	s.vinfo = (int64_t *)(p + off); off += R * 16;
	s.finfo = (int64_t *)(p + off); off += R * 16;
	s.cnt_v = (int64_t *)(p + off); off += R * 8;
	s.cnt_f = (int64_t *)(p + off); off += align16(R * 8);
	s.scan_tmp = p + off; off += align16(scan::tmp_bytes(R));
	s.words = (uint32_t *)(p + off); off += R * Nz * 4;
	s.bytes = off;
	return s;
}

static int check_args(const char *fn, const float *volume, uint32_t Nx, uint32_t Ny, uint32_t Nz, const void *scratch) {
	NR3D_CHECK(Nx >= 2 && Ny >= 2 && Nz >= 2, "%s: a volume of %u x %u x %u nodes, every dimension must be >= 2", fn, Nx, Ny, Nz);
	NR3D_CHECK((uint64_t)Nx * Ny < (1ull << 28), "%s: Nx Ny = %llu rows, fewer than 2^28 per call", fn, (unsigned long long)Nx * Ny);
	NR3D_CHECK((uint64_t)Nx * Ny * Nz < (1ull << 36), "%s: %llu nodes, fewer than 2^36 per call", fn, (unsigned long long)Nx * Ny * Nz);
	NR3D_CHECK(volume && scratch, "%s: NULL volume / scratch", fn);
	NR3D_CHECK(((uintptr_t)scratch & 7) == 0, "%s: scratch must be 8-byte aligned", fn);
	return 0;
}

}  // namespace mc
}  // namespace nr3d

using namespace nr3d;

extern "C" uint64_t nr3d_marching_cubes_scratch_bytes(uint32_t Nx, uint32_t Ny, uint32_t Nz) {
	return mc::carve(nullptr, Nx, Ny, Nz).bytes;
}

extern "C" int nr3d_marching_cubes_count(const float *volume, uint32_t Nx, uint32_t Ny, uint32_t Nz, float level, void *scratch,
                                         int64_t *totals, void *stream) {
	NR3D_TRY(mc::check_args("marching_cubes_count", volume, Nx, Ny, Nz, scratch));
	NR3D_CHECK(totals, "marching_cubes_count: NULL totals");
	const mc::Scratch s = mc::carve(scratch, Nx, Ny, Nz);
	const uint32_t R = Nx * Ny;
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(mc::k_rows<false>, dim3(div_up(R, mc::kWaves)), dim3(mc::kBlock), 0, st, volume, Nx, Ny, Nz, level, s.cnt_v, s.cnt_f,
	                   (const int64_t *)nullptr, (uint64_t)0, (float *)nullptr, (uint32_t *)nullptr);
	NR3D_LAUNCH_CHECK();
	NR3D_TRY((scan::pack_infos_from_counts<int64_t, int64_t>(R, s.cnt_v, s.vinfo, totals, s.scan_tmp, st)));
	NR3D_TRY((scan::pack_infos_from_counts<int64_t, int64_t>(R, s.cnt_f, s.finfo, totals + 1, s.scan_tmp, st)));
	return 0;
}

extern "C" int nr3d_marching_cubes_emit(const float *volume, uint32_t Nx, uint32_t Ny, uint32_t Nz, float level, void *scratch, uint64_t V,
                                        uint64_t F, float *verts, int64_t *faces, void *stream) {
	NR3D_TRY(mc::check_args("marching_cubes_emit", volume, Nx, Ny, Nz, scratch));
	if (V == 0) return 0;
	NR3D_CHECK(V < (1ull << 29), "marching_cubes_emit: V = %llu vertices, fewer than 2^29 per call (split the volume)", (unsigned long long)V);
	NR3D_CHECK(V <= 3ull * Nx * Ny * Nz && F <= 5ull * (Nx - 1) * (Ny - 1) * (Nz - 1), "marching_cubes_emit: V = %llu, F = %llu from %u x %u x %u nodes",
	           (unsigned long long)V, (unsigned long long)F, Nx, Ny, Nz);
	NR3D_CHECK(verts && (F == 0 || faces), "marching_cubes_emit: NULL verts / faces");
	const mc::Scratch s = mc::carve(scratch, Nx, Ny, Nz);
	const uint32_t R = Nx * Ny;
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(mc::k_rows<true>, dim3(div_up(R, mc::kWaves)), dim3(mc::kBlock), 0, st, volume, Nx, Ny, Nz, level, (int64_t *)nullptr,
	                   (int64_t *)nullptr, (const int64_t *)s.vinfo, V, verts, s.words);
	if (F) hipLaunchKernelGGL(mc::k_faces, dim3(div_up(R, mc::kWaves)), dim3(mc::kBlock), 0, st, volume, Nx, Ny, Nz, level,
	                          (const int64_t *)s.finfo, F, (const uint32_t *)s.words, faces);
	NR3D_LAUNCH_CHECK();
	return 0;
}
