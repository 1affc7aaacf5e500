// nr3d_lib_amd/csrc/pack_launch.h -- launchers of kernels that another translation unit chains behind its own, without the host in
// between.  pack_ops.hip's composites: occ_grid.hip (nr3d_march_composite_fwd / _bwd enqueue march -> scan -> emit -> composite) and
// neus_composite.hip.  ray_glue.hip's per-sample epilogue: occ_grid.hip (nr3d_ray_marching_emit enqueues it behind its second march).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nr3d {
namespace pk {

// fused alpha = 1 - exp(-sigma * delta) + alpha composite, one wave per ray over ALL rays of packed_info (int32 [n_rays, 2])
int launch_composite_rays_fwd(uint32_t n_rays, const int32_t *packed_info, const float *sigma, const float *delta, uint64_t sigma_rows,
                              const float *ts, const float *rgb, float eps, float thre, int normalize, float *alphas, float *vw,
                              float *mask, float *depth, float *rgb_out, hipStream_t st);
// ... with the marcher's cached emit in front, in the same launch (the wave of a ray copies its cached samples to their packed rows, then
// composites them)
int launch_emit_composite_rays_fwd(uint32_t n_rays, const int32_t *packed_info, const void *cache, uint32_t cache_stride,
                                   const float *rays_o, const float *rays_d, float *t_starts, float *t_ends, int32_t *ridx, int32_t *gidx,
                                   int64_t *ridx64, float *deltas, float *samples, const float *sigma, uint64_t sigma_rows,
                                   const float *rgb, float eps, float thre, int normalize, float *alphas, float *vw, float *mask,
                                   float *depth, float *rgb_out, hipStream_t st);
int launch_composite_rays_bwd(uint32_t n_rays, const int32_t *packed_info, const float *alphas, const float *vw, const float *ts,
                              const float *rgb, float eps, float thre, int normalize, const float *mask, const float *depth,
                              const float *g_mask, const float *g_depth, const float *g_rgb, float *grad_alphas, float *grad_t,
                              float *grad_rgb, const float *sigma, const float *delta, uint64_t sigma_rows, float *grad_sigma,
                              hipStream_t st);

// the packed composite with the samples' normals composited next to rgb (neus_composite.hip: nr3d_neus_composite_fwd / _bwd with nablas):
// the device bodies of nr3d_pack_composite_fwd / _bwd, one wave per pack; normals_mode 1 clamps nablas in place
int launch_neus_composite_packs_fwd(uint32_t P, const float *alphas, const float *ts, const float *rgb, float *nablas, int normals_mode,
                                    const int64_t *pack_infos, const int64_t *ray_index, float eps, float thre, int normalize, float *vw,
                                    float *mask, float *depth, float *rgb_out, float *normals_out, hipStream_t st);
int launch_neus_composite_packs_bwd(uint32_t P, const float *alphas, const float *vw, const float *ts, const float *rgb, const float *nablas,
                                    const int64_t *pack_infos, const int64_t *ray_index, float eps, float thre, int normalize,
                                    const float *mask, const float *depth, const float *g_mask, const float *g_depth, const float *g_rgb,
                                    const float *g_normals, const float *g_vw, float *grad_alphas, float *grad_t, float *grad_rgb,
                                    float *grad_nablas, hipStream_t st);

}  // namespace pk

namespace glue {

// the marcher's per-sample epilogue over S packed rows (occgrid_raymarch.py:87-112): ridx64 = (int64) ridx, deltas = t_ends - t_starts,
// samples [S, 3] = fma(rays_d[ridx], t_starts, rays_o[ridx]) (torch.addcmul); any output may be NULL
int launch_finish_samples(uint64_t S, const float *rays_o, const float *rays_d, const int32_t *ridx, const float *t_starts,
                          const float *t_ends, int64_t *ridx64, float *deltas, float *samples, hipStream_t st);

}  // namespace glue
}  // namespace nr3d
