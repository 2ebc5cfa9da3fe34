// kernels_output.hip -- the output transform on the device (rene_output_8bit, include/rene_hip.h): a [H][W][4] fp32 layer and its divisor in, tightly
// packed 8-bit pixels out, [H][W][3] or [H][W][4] with alpha 255 -- bit for bit the bytes of the host's rene_to_rgb8 / rene_to_aov8.  The device
// code -- the mean, the sRGB byte by the threshold table, the AOV transforms, the mapping of pixels to threads -- is output_pixel.h, which this unit
// shares with kernels_tonemap.hip; here are the transform x format kernels, the probe and the launchers.  Built with ROBUSTFLAGS (Makefile).
#include "output_pixel.h"

namespace rene {

template <int TRANSFORM, int FORMAT>
__global__ void __launch_bounds__(OUT_BLOCK) output_kernel(OutputLaunch L) {
  __shared__ float thr[TRANSFORM == RENE_OUTPUT_SRGB ? 256 : 1];
  output_pixels<TRANSFORM, FORMAT, TONEMAP_NONE>(L, 1.0f, 0.0f, thr);
}

// rene_output_probe: n values through output_byte, one lane each
template <int TRANSFORM>
__global__ void __launch_bounds__(OUT_BLOCK) output_probe_kernel(const float* __restrict__ v, uint8_t* __restrict__ out, size_t n, const float* __restrict__ thresholds) {
  __shared__ float thr[TRANSFORM == RENE_OUTPUT_SRGB ? 256 : 1];
  publish_threshold<TRANSFORM>(thr, fetch_threshold<TRANSFORM>(thresholds));
  const size_t i = (size_t)blockIdx.x * OUT_BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = (uint8_t)output_byte<TRANSFORM>(v[i], thr);
}

hipError_t launch_output(const OutputLaunch& L, int transform, int format, hipStream_t st) {
  const size_t n = (size_t)L.width * L.height;
  if (n == 0) return hipSuccess;
  const dim3 grid((unsigned)((n + (size_t)OUT_BLOCK * OUT_PIXELS - 1) / ((size_t)OUT_BLOCK * OUT_PIXELS))), block(OUT_BLOCK);
  const bool rgba = format == RENE_OUTPUT_RGBA8;
  switch (transform) {
    case RENE_OUTPUT_SRGB:
      if (rgba) hipLaunchKernelGGL((output_kernel<RENE_OUTPUT_SRGB, RENE_OUTPUT_RGBA8>), grid, block, 0, st, L);
      else hipLaunchKernelGGL((output_kernel<RENE_OUTPUT_SRGB, RENE_OUTPUT_RGB8>), grid, block, 0, st, L);
      break;
    case RENE_OUTPUT_AOV:
      if (rgba) hipLaunchKernelGGL((output_kernel<RENE_OUTPUT_AOV, RENE_OUTPUT_RGBA8>), grid, block, 0, st, L);
      else hipLaunchKernelGGL((output_kernel<RENE_OUTPUT_AOV, RENE_OUTPUT_RGB8>), grid, block, 0, st, L);
      break;
    case RENE_OUTPUT_AOV_NORMAL:
      if (rgba) hipLaunchKernelGGL((output_kernel<RENE_OUTPUT_AOV_NORMAL, RENE_OUTPUT_RGBA8>), grid, block, 0, st, L);
      else hipLaunchKernelGGL((output_kernel<RENE_OUTPUT_AOV_NORMAL, RENE_OUTPUT_RGB8>), grid, block, 0, st, L);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_output_probe(int transform, size_t n, const float* v, uint8_t* out, const float* thresholds, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 grid((unsigned)((n + OUT_BLOCK - 1) / OUT_BLOCK)), block(OUT_BLOCK);
  switch (transform) {
    case RENE_OUTPUT_SRGB: hipLaunchKernelGGL(output_probe_kernel<RENE_OUTPUT_SRGB>, grid, block, 0, st, v, out, n, thresholds); break;
    case RENE_OUTPUT_AOV: hipLaunchKernelGGL(output_probe_kernel<RENE_OUTPUT_AOV>, grid, block, 0, st, v, out, n, thresholds); break;
    case RENE_OUTPUT_AOV_NORMAL: hipLaunchKernelGGL(output_probe_kernel<RENE_OUTPUT_AOV_NORMAL>, grid, block, 0, st, v, out, n, thresholds); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace rene
