// chain_pass.h -- what the passes over the eight frame chains (device_scene.h, CHAINS) share on the device: kernels_noise.hip, kernels_robust.hip,
// kernels_features.hip, kernels_denoise_trim.hip and -- through atrous_filter.h -- kernels_denoise.hip include it; the output units (output_pixel.h, kernels_luminance.hip) take lum3 from it and nothing else.  Every decision two of them have to agree on is written here once;
// what only one of them does stays in its own file.
//
// The shape of a per-tile pass (the noise estimate, the robust resolve): one workgroup of PASS_BLOCK = 256 threads per OWNED tile k.  The tile's 1024
// pixel slots k * 1024 .. k * 1024 + 1023 are contiguous, thread j takes slots j, j + 256, j + 512, j + 768 -- consecutive lanes read consecutive
// 16-byte records -- and reads layer 0 of all eight chains for them: 32 independent 16-byte loads per thread, all issued before the first is waited
// for (load_layer0).  The feature export takes the same workgroup per owned tile with a pixel-major mapping of its own.
//
// The tile sums are reduced in a FIXED order (tile_reduce) -- a thread's four slots in slot order, a butterfly over the wave's 64 lanes, the four
// wave partials through LDS added in wave order by one lane -- and stored with one 16-byte vector store per tile: no atomics, so a tile's record is
// the same bit for bit from run to run, and the same in an unsharded context and in the tile shard that owns the tile.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rene {

constexpr uint32_t PASS_BLOCK = 256, PASS_PER_THREAD = TILE_SLOTS / PASS_BLOCK, PASS_WAVES = PASS_BLOCK / 64;

// the passes' luminance: (a + b) + c, which is what a + b + c means -- written out because two of the units fix every fp32 operation and its order
__device__ __forceinline__ float lum3(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

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

// slot r (0 .. 1023) of a tile -> the pixel's place (dx, dy) inside the tile: 8 x 8 sub-blocks, the inverse of tile_slot() (device_scene.h)
__device__ __forceinline__ uint2 slot_pixel(uint32_t r) {
  const uint32_t sub = r >> 6, l = r & 63u;
  return make_uint2((sub & 3u) * 8u + (l & 7u), (sub >> 2) * 8u + (l >> 3));
}

// where image tile `tile` starts, and owned tile k (image tile shard_rank + k * shard_count, the mapping of resolve_chains_kernel)
__device__ __forceinline__ uint2 image_tile_origin(const TileGrid& G, uint32_t tile) {
  return make_uint2((tile % G.tiles_x) * RENE_TILE_SIZE, (tile / G.tiles_x) * RENE_TILE_SIZE);
}
__device__ __forceinline__ uint2 owned_tile_origin(const TileGrid& G, uint32_t k) { return image_tile_origin(G, G.shard_rank + k * G.shard_count); }

// layer 0 of every chain for the calling thread's PASS_PER_THREAD slots of owned tile k (c[q]: slot threadIdx.x + q * PASS_BLOCK)
__device__ __forceinline__ void load_layer0(const float4* __restrict__ chains, const TileGrid& G, uint32_t k, float4 (&c)[PASS_PER_THREAD][CHAINS]) {
  const size_t n4 = (size_t)3 * G.n_slots, base = (size_t)k * TILE_SLOTS + threadIdx.x;
#pragma unroll
  for (uint32_t q = 0; q < PASS_PER_THREAD; ++q)
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) c[q][g] = chains[(size_t)g * n4 + base + q * PASS_BLOCK];
}

// the chain counts n_c of owned tile k: the launch's, or under adaptive sampling the tile's own set (workgroup-uniform: scalar loads)
__device__ __forceinline__ void tile_chain_counts(const ChainCounts& C, uint32_t k, uint32_t (&cn)[CHAINS]) {
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) cn[g] = C.chain_n[g];
  if (C.tile_set != nullptr) {
    const uint32_t* c = C.sets + (size_t)C.tile_set[k] * CHAINS;
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) cn[g] = c[g];
  }
}

// a thread's partial sums of its tile: NF floats and NU counters, reduced together behind one barrier (a pass without one kind asks for 0 of them:
// device code has no zero-length arrays, so the array keeps one element that nothing touches)
template <uint32_t NF, uint32_t NU>
struct TileSums {
  float f[NF ? NF : 1u];
  uint32_t u[NU ? NU : 1u];
};
// the fixed-order reduction over a workgroup of PASS_BLOCK threads; true in thread 0, whose `s` then holds the tile's totals.  LDS: the wave partials only
template <uint32_t NF, uint32_t NU>
__device__ __forceinline__ bool tile_reduce(TileSums<NF, NU>& s) {
  __shared__ float s_f[NF ? NF : 1u][PASS_WAVES];
  __shared__ uint32_t s_u[NU ? NU : 1u][PASS_WAVES];
#pragma unroll
  for (uint32_t i = 0; i < NF; ++i) s.f[i] = wave_sum(s.f[i]);
#pragma unroll
  for (uint32_t i = 0; i < NU; ++i) s.u[i] = wave_sum(s.u[i]);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (uint32_t i = 0; i < NF; ++i) s_f[i][wave] = s.f[i];
#pragma unroll
    for (uint32_t i = 0; i < NU; ++i) s_u[i][wave] = s.u[i];
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
#pragma unroll
  for (uint32_t i = 0; i < NF; ++i) {
    s.f[i] = s_f[i][0];
#pragma unroll
    for (uint32_t w = 1; w < PASS_WAVES; ++w) s.f[i] += s_f[i][w];
  }
#pragma unroll
  for (uint32_t i = 0; i < NU; ++i) {
    s.u[i] = s_u[i][0];
#pragma unroll
    for (uint32_t w = 1; w < PASS_WAVES; ++w) s.u[i] += s_u[i][w];
  }
  return true;
}

}  // namespace rene
