// kernels_denoise.hip -- the build-defined denoiser `atrous` (rene_denoise, include/rene_hip.h): an edge-avoiding a-trous wavelet filter
// (Dammertz et al. 2010; the spatial half of SVGF, Schied et al. 2017) guided by the first-hit normal and albedo layers and by the variance of
// the pixel's mean, which the eight frame chains (device_scene.h, CHAINS) give for nothing: eight independent sub-means per pixel.
//
//   prepare   one thread per owned pixel slot (chain_pass.h maps it to its pixel): reads the pixel's eight radiance records and the resolved guide layers, writes pixel-major records
//             rec[y][x] = {demodulated colour.rgb, variance of the mean of its luminance} and the constant guides g0 = {normal.xyz, albedo.r},
//             g1 = {albedo.g, albedo.b, 0, 0} (fp32: 16 + 32 bytes per pixel), and the unfiltered variance plane
//   pass      one launch per iteration i (step s = 2^i), one thread per pixel, 25 taps of three 16-byte loads each.  For small steps the
//             workgroup's 32 x 8 tile and a halo of 2 s pixels are staged in LDS (atrous_pass_kernel<S>, S > 0); the larger steps read their
//             taps through L2 (S == 0: consecutive lanes stay on consecutive records).  Both do the same arithmetic in the same order
//   finalize  remodulates and scales by the frame count: the unit of rene_download
//
// Nothing here writes the accumulation state: chains and image are read only.
#include <hip/hip_runtime.h>

#include "atrous_filter.h"

namespace rene {

// denoise_prepare_kernel and atrous_pass_kernel<S>: the text this unit shares with kernels_denoise_tiles.hip, here without per-tile constants and
// without the mask
#define ATROUS_TILES 0
#include "atrous_kernels.inc"
#undef ATROUS_TILES

__global__ void __launch_bounds__(256) denoise_finalize_kernel(const float4* __restrict__ rec, const float4* __restrict__ guides, float4* __restrict__ out, DenoiseLaunch D) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)D.grid.width * D.grid.height) return;
  const float4 c = rec[p], g0 = guides[2 * p], g1 = guides[2 * p + 1];
  out[p] = make_float4(c.x * (g0.w + D.albedo_floor) * D.n_frames, c.y * (g1.x + D.albedo_floor) * D.n_frames, c.z * (g1.y + D.albedo_floor) * D.n_frames, 0.0f);
}

hipError_t launch_denoise_prepare(const float* chains, const float* image, float* rec, float* guides, float* var_plane, const DenoiseLaunch& D, hipStream_t st) {
  if (D.grid.n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3((D.grid.n_slots + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<const float4*>(chains),
                     reinterpret_cast<const float4*>(image), reinterpret_cast<float4*>(rec), reinterpret_cast<float4*>(guides), var_plane, D);
  return hipGetLastError();
}

// steps up to `stage_max` go through the LDS-staged kernel.  The default is RENE_DENOISE_STAGE_MAX (-DRENE_DENOISE_STAGE_MAX=0 builds a library that
// never stages: the A/B of DESIGN.md section 4c); the environment variable of the same name overrides it per call (rene_hip.cpp)
#ifndef RENE_DENOISE_STAGE_MAX
#define RENE_DENOISE_STAGE_MAX 4
#endif
int denoise_stage_max() { return RENE_DENOISE_STAGE_MAX; }

hipError_t launch_atrous_pass(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, int stage_max, hipStream_t st) {
  const uint32_t tiles = ((D.grid.width + DN_TX - 1) / DN_TX) * ((D.grid.height + DN_TY - 1) / DN_TY);  // (at most 2^21 at 16384 x 16384)
  const dim3 grid((tiles + 7u) & ~7u), block(DN_BLOCK);
  const float4* r = reinterpret_cast<const float4*>(rec);
  const float4* g = reinterpret_cast<const float4*>(guides);
  float4* o = reinterpret_cast<float4*>(out);
  const uint32_t s = D.step <= (uint32_t)(stage_max < 0 ? 0 : stage_max) ? D.step : 0u;
  if (s == 1) hipLaunchKernelGGL(atrous_pass_kernel<1>, grid, block, 0, st, r, g, o, D);
  else if (s == 2) hipLaunchKernelGGL(atrous_pass_kernel<2>, grid, block, 0, st, r, g, o, D);
  else if (s == 4) hipLaunchKernelGGL(atrous_pass_kernel<4>, grid, block, 0, st, r, g, o, D);
  else hipLaunchKernelGGL(atrous_pass_kernel<0>, grid, block, 0, st, r, g, o, D);
  return hipGetLastError();
}

hipError_t launch_denoise_finalize(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, hipStream_t st) {
  const size_t n = (size_t)D.grid.width * D.grid.height;
  hipLaunchKernelGGL(denoise_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(rec),
                     reinterpret_cast<const float4*>(guides), reinterpret_cast<float4*>(out), D);
  return hipGetLastError();
}

}  // namespace rene
