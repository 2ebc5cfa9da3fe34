// kernels_denoise_trim.hip -- which chains the trimmed prepare of the `atrous` denoiser leaves out (rene_denoise_robust, rene_denoise_tiles_robust,
// include/rene_hip.h): steps R1 - R4 of that contract, which are steps 1 - 4 of rene_resolve_robust word for word, then the cap that keeps two chains.
//
//   one thread per owned pixel slot, the mapping of the denoiser's prepare: the eight layer-0 records are loaded before the arithmetic, and every
//   pixel inside the image gets one 4-byte word, trim[y][x] = j | kept << 8 (bit g of kept: chain g is kept).  The TRIM prepare of kernels_denoise.hip reads it.
//
// A unit of its own because of its flags.  The count j has to be bit for bit rene_resolve_robust's, whose arithmetic is specified operation by
// operation, and the prepare's records have to be bit for bit rene_denoise's, whose unit contracts multiply-adds and divides approximately.  No
// spelling of an operation escapes a unit's flags -- __fdiv_rn, __fmul_rn and __fadd_rn are the plain operators in this toolchain's headers -- so
// the two halves live in two units: this one is built like kernels_robust.hip (Makefile, ROBUSTFLAGS: no contraction, the correctly rounded
// division, denormals kept), and its text is that kernel's, with one slot per thread.
//
// Nothing here writes the accumulation state.  No atomics.
#include <hip/hip_runtime.h>

#include "chain_pass.h"

namespace rene {

__global__ void __launch_bounds__(256) denoise_trim_kernel(const float4* __restrict__ chains, uint32_t* __restrict__ trim, DenoiseTrimLaunch L) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // owned pixel slot (an unsharded context: tile = slot / 1024)
  if (i >= L.grid.n_slots) return;
  const uint32_t s = (uint32_t)i;
  const uint2 o = image_tile_origin(L.grid, s / TILE_SLOTS), d = slot_pixel(s % TILE_SLOTS);
  const uint32_t x = o.x + d.x, y = o.y + d.y;
  if (x >= L.grid.width || y >= L.grid.height) return;
  const size_t n4 = (size_t)3 * L.grid.n_slots, p = (size_t)y * L.grid.width + x;
  uint32_t cn[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) cn[g] = L.chain_n[g];
  if (L.tile_set != nullptr) {  // the counts of this workgroup's tile (workgroup-uniform: scalar loads)
    const uint32_t set = L.tile_set[blockIdx.x / (TILE_SLOTS / 256u)];
    if (set == NOISE_SET_NONE) {
      trim[p] = 0u;
      return;
    }
    const uint32_t* w = reinterpret_cast<const uint32_t*>(L.sets + (size_t)set * DENOISE_ROBUST_SET_FLOATS) + DENOISE_SET_FLOATS;
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) cn[g] = w[g];
  }
  uint32_t kk = 0;  // the chains that have received frames
  float nf[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    kk += cn[g] ? 1u : 0u;
    nf[g] = (float)cn[g];
  }
  // rene_resolve_robust's cap, then this contract's: at least two non-empty chains are kept
  const uint32_t j_cap = kk >= 2u ? min(min(L.max_trim, (kk - 1u) / 2u), (kk - 2u) / 2u) : 0u;
  const float kf = (float)kk, half_k = kf * 0.5f;
  float4 c[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) c[g] = chains[(size_t)g * n4 + i];  // layer 0 of chain g
  // R1 - R3: the chains' luminances, their ranks, the Gini coefficient
  float lc[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) lc[g] = cn[g] ? lum3(c[g].x / nf[g], c[g].y / nf[g], c[g].z / nf[g]) : 0.0f;
  uint32_t rank[CHAINS];
  float tot = 0.0f, num = 0.0f;
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    rank[g] = 0;
    if (!cn[g]) continue;
#pragma unroll
    for (uint32_t h = 0; h < CHAINS; ++h) {
      if (h == g || !cn[h]) continue;
      rank[g] += (lc[h] < lc[g] || (lc[h] == lc[g] && h < g)) ? 1u : 0u;
    }
    tot += lc[g];
    num += (float)((int)(2u * rank[g] + 1u) - (int)kk) * lc[g];
  }
  const float gini = tot > 0.0f ? num / (kf * tot) : 0.0f;
  // R4: how many chains go from either end (fmaxf / fminf: a NaN counts as 0, an infinity as the cap)
  const float t = (L.gain * gini) * half_k;
  const uint32_t j = min((uint32_t)fminf(fmaxf(t, 0.0f), 3.0f), j_cap);
  uint32_t kept = 0;
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) kept |= (!cn[g] || (rank[g] >= j && rank[g] < kk - j)) ? 1u << g : 0u;
  trim[p] = j | kept << 8;
}

hipError_t launch_denoise_trim(const float* chains, uint32_t* trim, const DenoiseTrimLaunch& L, hipStream_t st) {
  static_assert(TILE_SLOTS % 256u == 0, "a workgroup's slots lie inside one tile");
  if (L.grid.n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_trim_kernel, dim3((L.grid.n_slots + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<const float4*>(chains), trim, L);
  return hipGetLastError();
}

}  // namespace rene
