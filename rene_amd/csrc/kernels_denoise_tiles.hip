// kernels_denoise_tiles.hip -- the `atrous` denoiser tile by tile (rene_denoise_tiles, include/rene_hip.h): the filter of kernels_denoise.hip on an
// image whose 32 x 32 tiles stopped at different frame counts N_t (adaptive sampling, rene_set_active_tiles).  Steps 1 - 3 are per pixel and take the
// constants of the pixel's tile; steps 4 - 5 work on means and the variance of the mean and need no count at all, only to know which pixels take part.
//
//   prepare   as denoise_prepare_kernel, 256 consecutive slots per workgroup -- inside ONE owned tile, whose set of constants the workgroup reads
//             with scalar loads from the table the noise estimate's host code fills (one set per distinct N_t).  A pixel's validity and its tile's
//             count travel in the second guide record, whose .z and .w the taps load anyway and do not use: no new plane, no byte more per tap
//   pass      atrous_pass_tiles_kernel<S>: the text of atrous_pass_kernel<S> (atrous_kernels.inc) with the mask on -- same 32 x 8 tile, same halo, same
//             LDS layout, same order of the tiles over the XCDs.  An invalid pixel is a pixel outside the image
//   finalize  remodulates and scales by the pixel's own N_t; an invalid pixel hands out its unfiltered sum
//   mean      RENE_DENOISED_MEAN, on request: col * den of the last call's records, whichever of the two calls made them
//
// Nothing here writes the accumulation state: chains and image are read only.  No atomics.
#include <hip/hip_runtime.h>

#include "atrous_filter.h"

namespace rene {

// denoise_tiles_prepare_kernel and atrous_pass_tiles_kernel<S>: the text of kernels_denoise.hip's, with the per-tile constants and the mask
#define ATROUS_TILES 1
#include "atrous_kernels.inc"
#undef ATROUS_TILES

__global__ void __launch_bounds__(256) denoise_tiles_finalize_kernel(const float4* __restrict__ rec, const float4* __restrict__ guides, float4* __restrict__ out, DenoiseLaunch D) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)D.grid.width * D.grid.height) return;
  const float4 c = rec[p], g0 = guides[2 * p], g1 = guides[2 * p + 1];
  if (!dn_valid(g1)) {  // the unfiltered image: prepare left the pixel's sum here
    out[p] = make_float4(g0.x, g0.y, g0.z, 0.0f);
    return;
  }
  const float n = g1.w;  // (float)N_t
  out[p] = make_float4(c.x * (g0.w + D.albedo_floor) * n, c.y * (g1.x + D.albedo_floor) * n, c.z * (g1.y + D.albedo_floor) * n, 0.0f);
}

__global__ void __launch_bounds__(256) denoise_mean_kernel(const float4* __restrict__ rec, const float4* __restrict__ guides, float4* __restrict__ out, size_t n_px,
                                                           float albedo_floor, uint32_t masked) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_px) return;
  const float4 c = rec[p], g0 = guides[2 * p], g1 = guides[2 * p + 1];
  if (masked && !dn_valid(g1)) {
    out[p] = make_float4(g0.x, g0.y, g0.z, 0.0f);
    return;
  }
  out[p] = make_float4(c.x * (g0.w + albedo_floor), c.y * (g1.x + albedo_floor), c.z * (g1.y + albedo_floor), 0.0f);
}

hipError_t launch_denoise_tiles_prepare(const float* chains, const float* image, float* rec, float* guides, float* var_plane, const DenoiseLaunch& D,
                                        const DenoiseTileSets& T, hipStream_t st) {
  static_assert(TILE_SLOTS % DN_PREPARE_BLOCK == 0, "a prepare workgroup lies inside one tile");
  if (D.grid.n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_tiles_prepare_kernel, dim3((D.grid.n_slots + DN_PREPARE_BLOCK - 1u) / DN_PREPARE_BLOCK), dim3(DN_PREPARE_BLOCK), 0, st,
                     reinterpret_cast<const float4*>(chains), reinterpret_cast<const float4*>(image), reinterpret_cast<float4*>(rec), reinterpret_cast<float4*>(guides),
                     var_plane, D, T);
  return hipGetLastError();
}

hipError_t launch_atrous_tiles_pass(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, int stage_max, hipStream_t st) {
  const uint32_t tiles = ((D.grid.width + DN_TX - 1) / DN_TX) * ((D.grid.height + DN_TY - 1) / DN_TY);  // (at most 2^21 at 16384 x 16384)
  const dim3 grid((tiles + 7u) & ~7u), block(DN_BLOCK);
  const float4* r = reinterpret_cast<const float4*>(rec);
  const float4* g = reinterpret_cast<const float4*>(guides);
  float4* o = reinterpret_cast<float4*>(out);
  const uint32_t s = D.step <= (uint32_t)(stage_max < 0 ? 0 : stage_max) ? D.step : 0u;  // (launch_atrous_pass's choice)
  if (s == 1) hipLaunchKernelGGL(atrous_pass_tiles_kernel<1>, grid, block, 0, st, r, g, o, D);
  else if (s == 2) hipLaunchKernelGGL(atrous_pass_tiles_kernel<2>, grid, block, 0, st, r, g, o, D);
  else if (s == 4) hipLaunchKernelGGL(atrous_pass_tiles_kernel<4>, grid, block, 0, st, r, g, o, D);
  else hipLaunchKernelGGL(atrous_pass_tiles_kernel<0>, grid, block, 0, st, r, g, o, D);
  return hipGetLastError();
}

hipError_t launch_denoise_tiles_finalize(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, hipStream_t st) {
  const size_t n = (size_t)D.grid.width * D.grid.height;
  hipLaunchKernelGGL(denoise_tiles_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(rec),
                     reinterpret_cast<const float4*>(guides), reinterpret_cast<float4*>(out), D);
  return hipGetLastError();
}

hipError_t launch_denoise_mean(const float* rec, const float* guides, float* out, uint32_t width, uint32_t height, float albedo_floor, bool masked, hipStream_t st) {
  const size_t n = (size_t)width * height;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(rec),
                     reinterpret_cast<const float4*>(guides), reinterpret_cast<float4*>(out), n, albedo_floor, masked ? 1u : 0u);
  return hipGetLastError();
}

}  // namespace rene
