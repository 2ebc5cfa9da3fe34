// kernels_tonemap.hip -- rene_output_tonemapped (include/rene_hip.h): the output kernel of kernels_output.hip with exposure and a tone curve between
// the mean and its sRGB byte.  The kernel's body -- 4 consecutive pixels per thread, the loads ahead of the table's publication, the dword stores, the
// shard predicate -- is output_pixels (output_pixel.h), shared with that unit; the operator is its third template parameter.  A unit of its own, so
// that rene_output_8bit's kernels are the code they were: operator x format instantiations here, sRGB only.  Built with ROBUSTFLAGS: the curve's
// fp32 + x / are IEEE operations, none contracted, and the bytes are bit for bit those of the host's rene_tonemap_rgb8.
//   What an operator adds per pixel to 64 bytes in and 12 or 16 out per thread: 3 multiplies (exposure); Reinhard 2 divisions, 3 multiplies, the
//   luminance; ACES 3 divisions and 15 multiplies and adds.
#include "output_pixel.h"

namespace rene {

template <int OP, int FORMAT>
__global__ void __launch_bounds__(OUT_BLOCK) tonemap_kernel(TonemapLaunch L) {
  __shared__ float thr[256];
  output_pixels<RENE_OUTPUT_SRGB, FORMAT, OP>(L.out, L.scale, L.w2, thr);
}

// rene_tonemap_probe: n RGB triples through tonemap_pixel and output_byte, one lane each
template <int OP>
__global__ void __launch_bounds__(OUT_BLOCK) tonemap_probe_kernel(const float* __restrict__ rgb, uint8_t* __restrict__ out, size_t n, const float* __restrict__ thresholds, float scale,
                                                                  float w2) {
  __shared__ float thr[256];
  publish_threshold<RENE_OUTPUT_SRGB>(thr, fetch_threshold<RENE_OUTPUT_SRGB>(thresholds));
  const size_t i = (size_t)blockIdx.x * OUT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float3 c = tonemap_pixel<OP>(make_float3(rgb[3u * i], rgb[3u * i + 1u], rgb[3u * i + 2u]), scale, w2);
  out[3u * i] = (uint8_t)output_byte<RENE_OUTPUT_SRGB>(c.x, thr);
  out[3u * i + 1u] = (uint8_t)output_byte<RENE_OUTPUT_SRGB>(c.y, thr);
  out[3u * i + 2u] = (uint8_t)output_byte<RENE_OUTPUT_SRGB>(c.z, thr);
}

template <int OP>
static void launch_tonemap_op(const TonemapLaunch& L, bool rgba, dim3 grid, dim3 block, hipStream_t st) {
  if (rgba) hipLaunchKernelGGL((tonemap_kernel<OP, RENE_OUTPUT_RGBA8>), grid, block, 0, st, L);
  else hipLaunchKernelGGL((tonemap_kernel<OP, RENE_OUTPUT_RGB8>), grid, block, 0, st, L);
}

hipError_t launch_tonemap(const TonemapLaunch& L, int op, int format, hipStream_t st) {
  const size_t n = (size_t)L.out.width * L.out.height;
  if (n == 0) return hipSuccess;
  const dim3 grid((unsigned)((n + (size_t)OUT_BLOCK * OUT_PIXELS - 1) / ((size_t)OUT_BLOCK * OUT_PIXELS))), block(OUT_BLOCK);
  const bool rgba = format == RENE_OUTPUT_RGBA8;
  switch (op) {
    case RENE_TONEMAP_CLAMP: launch_tonemap_op<RENE_TONEMAP_CLAMP>(L, rgba, grid, block, st); break;
    case RENE_TONEMAP_REINHARD: launch_tonemap_op<RENE_TONEMAP_REINHARD>(L, rgba, grid, block, st); break;
    case RENE_TONEMAP_ACES: launch_tonemap_op<RENE_TONEMAP_ACES>(L, rgba, grid, block, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_tonemap_probe(int op, float scale, float w2, size_t n, const float* rgb, uint8_t* out, const float* thresholds, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 grid((unsigned)((n + OUT_BLOCK - 1) / OUT_BLOCK)), block(OUT_BLOCK);
  switch (op) {
    case RENE_TONEMAP_CLAMP: hipLaunchKernelGGL(tonemap_probe_kernel<RENE_TONEMAP_CLAMP>, grid, block, 0, st, rgb, out, n, thresholds, scale, w2); break;
    case RENE_TONEMAP_REINHARD: hipLaunchKernelGGL(tonemap_probe_kernel<RENE_TONEMAP_REINHARD>, grid, block, 0, st, rgb, out, n, thresholds, scale, w2); break;
    case RENE_TONEMAP_ACES: hipLaunchKernelGGL(tonemap_probe_kernel<RENE_TONEMAP_ACES>, grid, block, 0, st, rgb, out, n, thresholds, scale, w2); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace rene
