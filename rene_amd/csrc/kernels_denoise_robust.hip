// kernels_denoise_robust.hip -- the trimmed prepare of the `atrous` denoiser (rene_denoise_robust, rene_denoise_tiles_robust, include/rene_hip.h):
// the prepare of atrous_kernels.inc with steps 2 and 3 taken over the chains that kernels_denoise_trim.hip decided to keep.  The passes, finalize
// and the mean are the kernels of kernels_denoise.hip and kernels_denoise_tiles.hip, launched as they are.
//
//   one thread per owned pixel slot, 256 consecutive slots per workgroup, the eight layer-0 records loaded before the arithmetic -- the mapping
//   of the plain prepare -- plus one 4-byte word per pixel, trim[y][x] = j | kept << 8.
//
// Built with the denoiser's flags, and where j == 0 every expression is the plain prepare's, on the same constants in the same order: such a
// pixel's records are bit for bit rene_denoise's (rene_denoise_tiles').  Where j > 0 the pixel's own 1 / n_kept, n_c / n_kept and 1 / (h - 1)
// take the places of inv_n, chain_share and inv_km1; they are computed here, with this unit's division.
//
// Nothing here writes the accumulation state: chains, image and trim are read only.  No atomics.
#include <hip/hip_runtime.h>

#include "atrous_filter.h"

namespace rene {

// steps 1, 2', 3' for slot i = pixel p, with the constants of D; cn: the n_c behind D.chain_share; g1z, g1w: what the second guide carries
__device__ __forceinline__ void robust_prepare_pixel(const float4* __restrict__ chains, const float4* __restrict__ image, const uint32_t* __restrict__ trim,
                                                     float4* __restrict__ rec, float4* __restrict__ guides, float* __restrict__ var_plane, const DenoiseLaunch& D,
                                                     const uint32_t (&cn)[CHAINS], size_t i, size_t p, float g1z, float g1w) {
  const size_t n4 = (size_t)3 * D.grid.n_slots, np = (size_t)D.grid.width * D.grid.height;
  float4 c[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) c[g] = chains[(size_t)g * n4 + i];  // layer 0 of chain g
  const uint32_t w = trim[p], j = w & 0xffu, kept = w >> 8;
  // acc: the kept chains' sums in chain order, from C_0 or +0 (everything kept: ((c0 + c1) + c2) + ... like resolve_chains_kernel)
  float sr = (kept & 1u) ? c[0].x : 0.0f, sg = (kept & 1u) ? c[0].y : 0.0f, sb = (kept & 1u) ? c[0].z : 0.0f;
  uint32_t n_kept = (kept & 1u) ? cn[0] : 0u, kk = cn[0] ? 1u : 0u;
#pragma unroll
  for (uint32_t g = 1; g < CHAINS; ++g) {
    if (kept >> g & 1u) {
      sr += c[g].x;
      sg += c[g].y;
      sb += c[g].z;
      n_kept += cn[g];
    }
    kk += cn[g] ? 1u : 0u;
  }
  // the pixel's constants: the launch's where nothing is trimmed
  const float fk = (float)n_kept;
  const float inv_nk = j ? 1.0f / fk : D.inv_n, inv_hm1 = j ? 1.0f / (float)(kk - 2u * j - 1u) : D.inv_km1;
  const float4 s1 = image[np + p], s2 = image[2 * np + p];
  const float nx = s1.x * D.inv_n, ny = s1.y * D.inv_n, nz = s1.z * D.inv_n;
  const float ar = s2.x * D.inv_n, ag = s2.y * D.inv_n, ab = s2.z * D.inv_n;
  const float ir = 1.0f / (ar + D.albedo_floor), ig = 1.0f / (ag + D.albedo_floor), ib = 1.0f / (ab + D.albedo_floor);
  const float dr = sr * inv_nk * ir, dg = sg * inv_nk * ig, db = sb * inv_nk * ib;
  const float lm = lum3(dr, dg, db);
  float var = 0.0f;
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    if ((kept >> g & 1u) && D.chain_share[g] > 0.0f) {  // kept chains that have received frames
      const float share = j ? (float)cn[g] / fk : D.chain_share[g];
      const float t = lum3(c[g].x * D.chain_inv[g] * ir, c[g].y * D.chain_inv[g] * ig, c[g].z * D.chain_inv[g] * ib) - lm;
      var += share * (t * t);
    }
  }
  var *= inv_hm1;
  rec[p] = make_float4(dr, dg, db, var);
  guides[2 * p] = make_float4(nx, ny, nz, ar);
  guides[2 * p + 1] = make_float4(ag, ab, g1z, g1w);
  var_plane[p] = var;
}

__global__ void __launch_bounds__(256) denoise_robust_prepare_kernel(const float4* __restrict__ chains, const float4* __restrict__ image, const uint32_t* __restrict__ trim,
                                                                     float4* __restrict__ rec, float4* __restrict__ guides, float* __restrict__ var_plane, DenoiseLaunch D,
                                                                     DenoiseChainCounts N) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // owned pixel slot (an unsharded context: tile = slot / 1024)
  if (i >= D.grid.n_slots) return;
  const uint32_t s = (uint32_t)i;
  const uint2 o = image_tile_origin(D.grid, s / TILE_SLOTS), d = slot_pixel(s % TILE_SLOTS);
  const uint32_t x = o.x + d.x, y = o.y + d.y;
  if (x >= D.grid.width || y >= D.grid.height) return;
  robust_prepare_pixel(chains, image, trim, rec, guides, var_plane, D, N.chain_n, i, (size_t)y * D.grid.width + x, 0.0f, 0.0f);
}

__global__ void __launch_bounds__(256) denoise_tiles_robust_prepare_kernel(const float4* __restrict__ chains, const float4* __restrict__ image, const uint32_t* __restrict__ trim,
                                                                           float4* __restrict__ rec, float4* __restrict__ guides, float* __restrict__ var_plane, DenoiseLaunch D,
                                                                           DenoiseTileSets T) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= D.grid.n_slots) return;
  const uint32_t s = (uint32_t)i;
  const uint2 o = image_tile_origin(D.grid, s / TILE_SLOTS), d = slot_pixel(s % TILE_SLOTS);
  const uint32_t x = o.x + d.x, y = o.y + d.y;
  if (x >= D.grid.width || y >= D.grid.height) return;
  const size_t p = (size_t)y * D.grid.width + x;
  // the constants of this workgroup's tile: its 256 consecutive slots lie inside one owned tile (workgroup-uniform: scalar loads)
  const uint32_t set = T.tile_set[blockIdx.x / (TILE_SLOTS / 256u)];
  if (set == NOISE_SET_NONE) {  // as denoise_tiles_prepare_kernel: finite records, and the unfiltered sum where finalize finds it
    const float4 s0 = image[p];
    rec[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    guides[2 * p] = make_float4(s0.x, s0.y, s0.z, 0.0f);
    guides[2 * p + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    var_plane[p] = 0.0f;
    return;
  }
  const float* k = T.sets + (size_t)set * DENOISE_ROBUST_SET_FLOATS;
  D.inv_n = k[0];
  D.inv_km1 = k[1];
  uint32_t cn[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    D.chain_share[g] = k[2u + g];
    D.chain_inv[g] = k[2u + CHAINS + g];
    cn[g] = __float_as_uint(k[DENOISE_SET_FLOATS + g]);
  }
  D.n_frames = k[NOISE_SET_FLOATS];
  robust_prepare_pixel(chains, image, trim, rec, guides, var_plane, D, cn, i, p, 1.0f, D.n_frames);  // valid, (float)N_t: where the taps load them
}

hipError_t launch_denoise_robust_prepare(const float* chains, const float* image, const uint32_t* trim, float* rec, float* guides, float* var_plane,
                                         const DenoiseLaunch& D, const DenoiseChainCounts& N, hipStream_t st) {
  if (D.grid.n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_robust_prepare_kernel, dim3((D.grid.n_slots + DN_PREPARE_BLOCK - 1u) / DN_PREPARE_BLOCK), dim3(DN_PREPARE_BLOCK), 0, st,
                     reinterpret_cast<const float4*>(chains), reinterpret_cast<const float4*>(image), trim, reinterpret_cast<float4*>(rec),
                     reinterpret_cast<float4*>(guides), var_plane, D, N);
  return hipGetLastError();
}

hipError_t launch_denoise_tiles_robust_prepare(const float* chains, const float* image, const uint32_t* trim, float* rec, float* guides, float* var_plane,
                                               const DenoiseLaunch& D, const DenoiseTileSets& T, hipStream_t st) {
  static_assert(TILE_SLOTS % DN_PREPARE_BLOCK == 0, "a prepare workgroup lies inside one tile");
  if (D.grid.n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_tiles_robust_prepare_kernel, dim3((D.grid.n_slots + DN_PREPARE_BLOCK - 1u) / DN_PREPARE_BLOCK), dim3(DN_PREPARE_BLOCK), 0, st,
                     reinterpret_cast<const float4*>(chains), reinterpret_cast<const float4*>(image), trim, reinterpret_cast<float4*>(rec),
                     reinterpret_cast<float4*>(guides), var_plane, D, T);
  return hipGetLastError();
}

}  // namespace rene
