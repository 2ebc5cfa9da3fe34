// kernels_noise.hip -- the noise estimate (rene_estimate_noise, include/rene_hip.h): per owned 32 x 32 tile, the sum of the pixels' variance of the
// mean and the sum of their luminance, both taken from the eight frame chains (device_scene.h, CHAINS) exactly as the denoiser's step 3 takes
// them with den = 1.  The host turns the tile records into the tile and image figures in fp64.
//
//   one workgroup of 256 threads per OWNED tile k, in the slot-major mapping of chain_pass.h: every thread holds layer 0 of all eight chains for
//   its four slots before the arithmetic starts.
//
// The sums are reduced in the FIXED order of chain_pass.h (tile_reduce) and stored with one 16-byte vector store per tile: no atomics, so a tile's
// record is the same bit for bit from run to run, and the same in an unsharded context and in the tile shard that owns the tile.
//
// Nothing here writes the accumulation state: the chains are read only, the resolved image is not needed.
//
// Adaptive sampling (rene_set_active_tiles): where the owned tiles differ in their frame counts N_t, the constants of the estimate -- 1 / N, 1 / (k - 1),
// n_c / N, 1 / n_c -- differ per tile.  The host computes one set per distinct N_t with the very code that fills NoiseLaunch for a uniform context and
// hands over a table of sets and a set index per owned tile (NoiseLaunch::sets, ::tile_set; NOISE_SET_NONE: the tile has frames in fewer than two
// chains, its record is zero).  The kernel replaces its constants by the tile's set before the arithmetic, which is the same code on the same
// numbers as in a uniform context of N_t frames: the tile's record is that context's bit for bit.  Without a table nothing is read.
#include <hip/hip_runtime.h>

#include "chain_pass.h"

namespace rene {

__global__ void __launch_bounds__(PASS_BLOCK) noise_tiles_kernel(const float4* __restrict__ chains, float4* __restrict__ tiles, NoiseLaunch L) {
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
  const uint2 o = owned_tile_origin(L.grid, k);
  float4 c[PASS_PER_THREAD][CHAINS];
  load_layer0(chains, L.grid, k, c);
  TileSums<2, 1> s{};  // {sum of the variance of the mean, sum of the luminance}, {pixels inside the image}
#pragma unroll
  for (uint32_t q = 0; q < PASS_PER_THREAD; ++q) {
    const uint2 d = slot_pixel(threadIdx.x + q * PASS_BLOCK);
    const uint32_t x = o.x + d.x, y = o.y + d.y;
    if (x >= L.grid.width || y >= L.grid.height) continue;  // a ragged tile's slots outside the image contribute nothing
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
    s.f[0] += var * L.inv_km1;
    s.f[1] += lm;
    s.u[0] += 1u;
  }
  if (tile_reduce(s)) tiles[k] = make_float4(s.f[0], s.f[1], __uint_as_float(s.u[0]), 0.0f);  // one 16-byte vector store per tile
}

hipError_t launch_noise_tiles(const float* chains, float* tiles, const NoiseLaunch& L, hipStream_t st) {
  const uint32_t n_owned = L.grid.n_slots / TILE_SLOTS;
  if (n_owned == 0) return hipSuccess;
  hipLaunchKernelGGL(noise_tiles_kernel, dim3(n_owned), dim3(PASS_BLOCK), 0, st, reinterpret_cast<const float4*>(chains), reinterpret_cast<float4*>(tiles), L);
  return hipGetLastError();
}

}  // namespace rene
