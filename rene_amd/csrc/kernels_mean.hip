// kernels_mean.hip -- rene_download_mean (include/rene_hip.h): a layer of the resolved image divided by the frames its tiles have received.
//
// Under adaptive sampling (rene_set_active_tiles) the owned tiles differ in their frame counts N_t, and the image a caller wants is the mean, every
// pixel over its own tile's N_t.  One thread per texel of the layer, 16 bytes in and out; the tile's count is one cached load shared by the
// 32 x 32 texels of the tile.
//
// This unit is compiled WITHOUT the two options the render kernels take for speed (Makefile, MEANFLAGS): `/` below is the correctly rounded IEEE
// fp32 division, denormals kept -- on a context whose tiles all hold N frames the result is bit for bit rene_download's sums / (float)N as a host
// computes it.  (The render units' `/` is v_rcp_f32 and a multiply.)
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rene {

namespace {
constexpr uint32_t MEAN_BLOCK = 256;
}

__global__ void __launch_bounds__(MEAN_BLOCK) tile_mean_kernel(const float4* __restrict__ layer, float4* __restrict__ out, const uint32_t* __restrict__ tile_frames,
                                                               uint32_t W, uint32_t H, uint32_t tiles_x) {
  const size_t i = (size_t)blockIdx.x * MEAN_BLOCK + threadIdx.x;  // y * W + x
  if (i >= (size_t)W * H) return;
  const uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i - (size_t)y * W);
  const uint32_t n = tile_frames[(y / RENE_TILE_SIZE) * tiles_x + x / RENE_TILE_SIZE];
  float4 v = layer[i];
  if (n == 0u) {
    v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  } else {
    const float d = (float)n;
    v.x = v.x / d;
    v.y = v.y / d;
    v.z = v.z / d;
    v.w = 0.0f;
  }
  out[i] = v;
}

hipError_t launch_tile_mean(const float* layer, float* out, const uint32_t* tile_frames, uint32_t width, uint32_t height, uint32_t tiles_x, hipStream_t st) {
  const size_t n = (size_t)width * height;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(tile_mean_kernel, dim3((unsigned)((n + MEAN_BLOCK - 1) / MEAN_BLOCK)), dim3(MEAN_BLOCK), 0, st, reinterpret_cast<const float4*>(layer),
                     reinterpret_cast<float4*>(out), tile_frames, width, height, tiles_x);
  return hipGetLastError();
}

}  // namespace rene
