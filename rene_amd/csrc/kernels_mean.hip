// kernels_mean.hip -- the resolve of the frame chains into the image a call hands out (rene_download, rene_framebuffer: resolve_chains_kernel), and
// rene_download_mean (include/rene_hip.h): a layer of the resolved image divided by the frames its tiles have received.
//
// Under adaptive sampling (rene_set_active_tiles) the owned tiles differ in their frame counts N_t, and the image a caller wants is the mean, every
// pixel over its own tile's N_t.  One thread per texel of the layer, 16 bytes in and out; the tile's count is one cached load shared by the
// 32 x 32 texels of the tile.
//
// This unit is compiled WITHOUT the two options the render kernels take for speed (Makefile, MEANFLAGS): `/` below is the correctly rounded IEEE
// fp32 division, denormals kept -- on a context whose tiles all hold N frames the result is bit for bit rene_download's sums / (float)N as a host
// computes it, and the resolved sums are ((c0 + c1) + ...) + c7 as a host computes them, a denormal or a -0.0 included.  (The render units' `/` is
// v_rcp_f32 and a multiply, and their additions flush denormals.)
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

// frame chains (device_scene.h, CHAINS): the image a call hands out = the chains' records added in chain order, ((c0 + c1) + c2) + ..., written to the
// pixel's place in the [3][H][W][4] image -- the chains themselves are left as they are (they go on accumulating across launches); the alpha channel
// of the output is 0 (lib.rs:170 never writes it; in the chains' records it holds their versions).  One thread per (layer, owned pixel slot), 16 bytes
// each: the chains are read in slot order, the image written in runs of eight texels; only the tiles the context owns are written (a tile shard
// leaves the rest of the image as it is), and slots of a ragged tile outside the image are skipped.  It is in THIS unit for its flags: the render
// units flush fp32 denormals (Makefile, HIPFLAGS), and there the additions below turned a denormal chain sum into 0 -- while the robust resolve and
// the feature export, which add the same chains with denormals kept, promise pixels that are bit for bit rene_download_mean's.
__global__ void __launch_bounds__(MEAN_BLOCK) resolve_chains_kernel(const float4* chains, float4* out, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_slots,
                                                               uint32_t shard_rank, uint32_t shard_count) {
  const size_t i = (size_t)blockIdx.x * MEAN_BLOCK + threadIdx.x;  // layer * n_slots + slot
  const size_t n4 = (size_t)3 * n_slots;
  if (i >= n4) return;
  const uint32_t layer = (uint32_t)(i / n_slots), s = (uint32_t)(i - (size_t)layer * n_slots);
  const uint32_t tile = shard_rank + (s >> 10) * shard_count, r = s & 1023u, sub = r >> 6, l = r & 63u;
  const uint32_t x = (tile % tiles_x) * RENE_TILE_SIZE + (sub & 3u) * 8u + (l & 7u), y = (tile / tiles_x) * RENE_TILE_SIZE + (sub >> 2) * 8u + (l >> 3);
  if (x >= W || y >= H) return;
  float4 a = chains[i];
#pragma unroll
  for (uint32_t g = 1; g < CHAINS; ++g) {
    const float4 b = chains[(size_t)g * n4 + i];
    a.x += b.x;
    a.y += b.y;
    a.z += b.z;
  }
  a.w = 0.0f;
  out[((size_t)layer * H + y) * W + x] = a;
}
hipError_t launch_resolve_chains(const float* chains, float* out, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t n_slots, uint32_t shard_rank,
                                 uint32_t shard_count, hipStream_t st) {
  const size_t n = (size_t)3 * n_slots;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(resolve_chains_kernel, dim3((unsigned)((n + MEAN_BLOCK - 1) / MEAN_BLOCK)), dim3(MEAN_BLOCK), 0, st, reinterpret_cast<const float4*>(chains),
                     reinterpret_cast<float4*>(out), width, height, tiles_x, n_slots, shard_rank, shard_count);
  return hipGetLastError();
}

hipError_t launch_tile_mean(const float* layer, float* out, const uint32_t* tile_frames, uint32_t width, uint32_t height, uint32_t tiles_x, hipStream_t st) {
  const size_t n = (size_t)width * height;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(tile_mean_kernel, dim3((unsigned)((n + MEAN_BLOCK - 1) / MEAN_BLOCK)), dim3(MEAN_BLOCK), 0, st, reinterpret_cast<const float4*>(layer),
                     reinterpret_cast<float4*>(out), tile_frames, width, height, tiles_x);
  return hipGetLastError();
}

}  // namespace rene
