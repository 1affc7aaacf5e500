// nr3d_lib_amd/csrc/unit_normal.h -- a sample's normal vector as the NeuS render composite reads it, shared by the rows' kernels
// (neus_composite.hip) and the packs' (pack_ops.hip, NRM) so that the two layouts cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

namespace nr3d {

struct V3 { float x, y, z; };

// torch's clamp(-1, 1): a NaN stays one
__device__ __forceinline__ float clamp_unit(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }

// nablas[i] for the composite.  mode 0 (training): as stored.  mode 1 (evaluation): clamped to [-1, 1] and STORED BACK (the reference's
// clamp_ is in place), then c / max(|c|, 1e-12) as F.normalize gives it; a zero vector stays zero.
__device__ __forceinline__ V3 load_normal(float *nablas, size_t i, int mode) {
	V3 v = {nablas[3 * i], nablas[3 * i + 1], nablas[3 * i + 2]};
	if (mode) {
		v.x = clamp_unit(v.x); v.y = clamp_unit(v.y); v.z = clamp_unit(v.z);
		nablas[3 * i] = v.x; nablas[3 * i + 1] = v.y; nablas[3 * i + 2] = v.z;
		const float d = fmaxf(sqrtf(v.x * v.x + v.y * v.y + v.z * v.z), 1e-12f);
		v.x /= d; v.y /= d; v.z /= d;
	}
	return v;
}

}  // namespace nr3d
