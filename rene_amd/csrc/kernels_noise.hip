// kernels_noise.hip -- the noise estimate (rene_estimate_noise, include/rene_hip.h): per owned 32 x 32 tile, the sum of the pixels' variance of the
// mean and the sum of their luminance, both taken from the eight frame chains (device_scene.h, CHAINS) exactly as the denoiser's step 3 takes
// them with den = 1.  The host turns the tile records into the tile and image figures in fp64.
//
//   one workgroup of 256 threads per OWNED tile k (image tile shard_rank + k * shard_count, the mapping of resolve_chains_kernel): the tile's
//   1024 pixel slots k * 1024 .. k * 1024 + 1023 are contiguous, thread j takes slots j, j + 256, j + 512, j + 768 -- consecutive lanes read
//   consecutive 16-byte records -- and reads layer 0 of all eight chains for them: 32 independent 16-byte loads per thread.
//
// The sums are reduced in a FIXED order -- a thread's four slots in slot order, a butterfly over the wave's 64 lanes, the four wave partials
// through LDS added in wave order by one lane -- and stored with one 16-byte vector store per tile: no atomics, so a tile's record is the same
// bit for bit from run to run, and the same in an unsharded context and in the tile shard that owns the tile.
//
// Nothing here writes the accumulation state: the chains are read only, the resolved image is not needed.
//
// Adaptive sampling (rene_set_active_tiles): where the owned tiles differ in their frame counts N_t, the constants of the estimate -- 1 / N, 1 / (k - 1),
// n_c / N, 1 / n_c -- differ per tile.  The host computes one set per distinct N_t with the very code that fills NoiseLaunch for a uniform context and
// hands over a table of sets and a set index per owned tile (NoiseLaunch::sets, ::tile_set; NOISE_SET_NONE: the tile has frames in fewer than two
// chains, its record is zero).  The kernel replaces its constants by the tile's set before the arithmetic, which is the same code on the same
// numbers as in a uniform context of N_t frames: the tile's record is that context's bit for bit.  Without a table nothing is read.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rene {

namespace {

constexpr uint32_t NOISE_BLOCK = 256, NOISE_PER_THREAD = TILE_SLOTS / NOISE_BLOCK, NOISE_WAVES = NOISE_BLOCK / 64;

__device__ __forceinline__ float lum3(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

// every lane ends with the same bits: at each level both partners add the same two numbers, and fp32 addition commutes
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  return v;
}

}  // namespace

__global__ void __launch_bounds__(NOISE_BLOCK) noise_tiles_kernel(const float4* __restrict__ chains, float4* __restrict__ tiles, NoiseLaunch L) {
  __shared__ float s_var[NOISE_WAVES], s_lum[NOISE_WAVES];
  __shared__ uint32_t s_n[NOISE_WAVES];
  const uint32_t k = blockIdx.x;  // owned tile (the grid is exactly the owned tiles: k * 1024 + 1023 < n_slots)
  if (L.tile_set != nullptr) {  // per-tile constants (workgroup-uniform: scalar loads)
    const uint32_t set = L.tile_set[k];
    if (set == NOISE_SET_NONE) {
      if (threadIdx.x == 0) tiles[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      return;
    }
    const float* c = L.sets + (size_t)set * NOISE_SET_FLOATS;
    L.inv_n = c[0];
    L.inv_km1 = c[1];
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) {
      L.chain_share[g] = c[2u + g];
      L.chain_inv[g] = c[2u + CHAINS + g];
    }
  }
  const uint32_t tile = L.shard_rank + k * L.shard_count;
  const uint32_t x0 = (tile % L.tiles_x) * RENE_TILE_SIZE, y0 = (tile / L.tiles_x) * RENE_TILE_SIZE;
  const size_t n4 = (size_t)3 * L.n_slots, base = (size_t)k * TILE_SLOTS + threadIdx.x;
  float4 c[NOISE_PER_THREAD][CHAINS];
#pragma unroll
  for (uint32_t q = 0; q < NOISE_PER_THREAD; ++q)
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) c[q][g] = chains[(size_t)g * n4 + base + q * NOISE_BLOCK];  // layer 0 of chain g
  float a = 0.0f, b = 0.0f;
  uint32_t n = 0;
#pragma unroll
  for (uint32_t q = 0; q < NOISE_PER_THREAD; ++q) {
    const uint32_t r = threadIdx.x + q * NOISE_BLOCK, sub = r >> 6, l = r & 63u;
    const uint32_t x = x0 + (sub & 3u) * 8u + (l & 7u), y = y0 + (sub >> 2) * 8u + (l >> 3);
    if (x >= L.width || y >= L.height) continue;  // a ragged tile's slots outside the image contribute nothing
    float sr = c[q][0].x, sg = c[q][0].y, sb = c[q][0].z;  // ((c0 + c1) + c2) + ... like resolve_chains_kernel
#pragma unroll
    for (uint32_t g = 1; g < CHAINS; ++g) {
      sr += c[q][g].x;
      sg += c[q][g].y;
      sb += c[q][g].z;
    }
    const float lm = lum3(sr * L.inv_n, sg * L.inv_n, sb * L.inv_n);
    float var = 0.0f;
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) {
      if (L.chain_share[g] > 0.0f) {  // chains that have received frames
        const float t = lum3(c[q][g].x * L.chain_inv[g], c[q][g].y * L.chain_inv[g], c[q][g].z * L.chain_inv[g]) - lm;
        var += L.chain_share[g] * (t * t);
      }
    }
    a += var * L.inv_km1;
    b += lm;
    n += 1u;
  }
  a = wave_sum(a);
  b = wave_sum(b);
  n = wave_sum(n);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
    s_var[wave] = a;
    s_lum[wave] = b;
    s_n[wave] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = s_var[0], tb = s_lum[0];
    uint32_t tn = s_n[0];
#pragma unroll
    for (uint32_t w = 1; w < NOISE_WAVES; ++w) {
      ta += s_var[w];
      tb += s_lum[w];
      tn += s_n[w];
    }
    tiles[k] = make_float4(ta, tb, __uint_as_float(tn), 0.0f);  // one 16-byte vector store per tile
  }
}

hipError_t launch_noise_tiles(const float* chains, float* tiles, const NoiseLaunch& L, hipStream_t st) {
  const uint32_t n_owned = L.n_slots / TILE_SLOTS;
  if (n_owned == 0) return hipSuccess;
  hipLaunchKernelGGL(noise_tiles_kernel, dim3(n_owned), dim3(NOISE_BLOCK), 0, st, reinterpret_cast<const float4*>(chains), reinterpret_cast<float4*>(tiles), L);
  return hipGetLastError();
}

}  // namespace rene
