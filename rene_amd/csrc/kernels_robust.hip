// kernels_robust.hip -- the firefly-robust resolve (rene_resolve_robust, include/rene_hip.h): per owned pixel the trimmed mean over the eight frame
// chains (device_scene.h, CHAINS), how many chains are trimmed following from the Gini coefficient of the chains' luminances; per owned 32 x 32
// tile the sums of the plain and of the robust mean's luminance, so that the caller sees what the trimming removed.
//
//   one workgroup of 256 threads per OWNED tile k, in the slot-major mapping of chain_pass.h: every thread holds layer 0 of all eight chains for
//   its four slots before the arithmetic starts; each thread writes one 16-byte vector store per pixel, {rgb, (float)j}, into the pixel-major
//   [H][W][4] output.
//
// The specification fixes every fp32 operation and its order, so this unit is compiled with -ffp-contract=off (no fused multiply-add is formed)
// and, like kernels_mean.hip, without the two options that trade the correctly rounded division and the denormals for speed (Makefile,
// ROBUSTFLAGS): the pixels are bit for bit the numpy restatement's (tests/robust_reference.py), and where nothing is trimmed rene_download_mean's.
//
// The tile sums are reduced in the FIXED order of chain_pass.h (tile_reduce) and stored with one 16-byte vector store per tile: no atomics.
//
// Adaptive sampling: where the owned tiles differ in their frame counts the host hands over the chain counts n_c of every distinct N_t and a set
// index per owned tile (ChainCounts::sets, ::tile_set); the kernel takes the tile's counts (tile_chain_counts) before the arithmetic.
//
// Nothing here writes the accumulation state.
#include <hip/hip_runtime.h>

#include "chain_pass.h"

namespace rene {

__global__ void __launch_bounds__(PASS_BLOCK) robust_tiles_kernel(const float4* __restrict__ chains, float4* __restrict__ out, float4* __restrict__ tiles, RobustLaunch L) {
  const uint32_t k = blockIdx.x;  // owned tile (the grid is exactly the owned tiles: k * 1024 + 1023 < n_slots)
  uint32_t cn[CHAINS];
  tile_chain_counts(L.counts, k, cn);
  uint32_t n_total = 0, kk = 0;  // N_t and the chains that have received frames
  float nf[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    n_total += cn[g];
    kk += cn[g] ? 1u : 0u;
    nf[g] = (float)cn[g];
  }
  const uint32_t j_cap = kk ? min(L.max_trim, (kk - 1u) / 2u) : 0u;
  const float kf = (float)kk, half_k = kf * 0.5f, n_total_f = (float)n_total;
  const uint2 o = owned_tile_origin(L.grid, k);
  float4 c[PASS_PER_THREAD][CHAINS];
  load_layer0(chains, L.grid, k, c);
  TileSums<2, 2> s{};  // {sum of lum(plain mean), sum of lum(robust mean)}, {pixels inside the image, pixels with j > 0}
#pragma unroll
  for (uint32_t q = 0; q < PASS_PER_THREAD; ++q) {
    const uint2 d = slot_pixel(threadIdx.x + q * PASS_BLOCK);
    const uint32_t x = o.x + d.x, y = o.y + d.y;
    if (x >= L.grid.width || y >= L.grid.height) continue;  // a ragged tile's slots outside the image: nothing is written, nothing counted
    float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float lum_plain = 0.0f, lum_robust = 0.0f;
    if (n_total != 0) {
      // steps 1 to 3: the chains' luminances, their ranks, the Gini coefficient
      float lc[CHAINS];
#pragma unroll
      for (uint32_t g = 0; g < CHAINS; ++g) lc[g] = cn[g] ? lum3(c[q][g].x / nf[g], c[q][g].y / nf[g], c[q][g].z / nf[g]) : 0.0f;
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
      // step 4: how many chains go from either end (fmaxf / fminf: a NaN counts as 0, an infinity as the cap)
      const float t = (L.gain * gini) * half_k;
      const uint32_t j = min((uint32_t)fminf(fmaxf(t, 0.0f), 3.0f), j_cap);
      // step 5: the kept chains' sum over their frames; S0 in the same order for the plain mean
      float ar = 0.0f, ag = 0.0f, ab = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
      uint32_t n_kept = 0;
#pragma unroll
      for (uint32_t g = 0; g < CHAINS; ++g) {
        sr += c[q][g].x;
        sg += c[q][g].y;
        sb += c[q][g].z;
        const bool kept = !cn[g] || (rank[g] >= j && rank[g] < kk - j);
        if (kept) {
          ar += c[q][g].x;
          ag += c[q][g].y;
          ab += c[q][g].z;
          n_kept += cn[g];
        }
      }
      const float nk = (float)n_kept;  // j <= (k - 1) / 2: at least one non-empty chain is kept
      res = make_float4(ar / nk, ag / nk, ab / nk, (float)j);
      lum_robust = lum3(res.x, res.y, res.z);
      lum_plain = lum3(sr / n_total_f, sg / n_total_f, sb / n_total_f);
      s.u[1] += j ? 1u : 0u;
    }
    out[(size_t)y * L.grid.width + x] = res;  // one 16-byte vector store per pixel
    s.f[0] += lum_plain;
    s.f[1] += lum_robust;
    s.u[0] += 1u;
  }
  if (tile_reduce(s)) tiles[k] = make_float4(s.f[0], s.f[1], __uint_as_float(s.u[0]), __uint_as_float(s.u[1]));  // one 16-byte vector store per tile
}

hipError_t launch_robust_tiles(const float* chains, float* out, float* tiles, const RobustLaunch& L, hipStream_t st) {
  const uint32_t n_owned = L.grid.n_slots / TILE_SLOTS;
  if (n_owned == 0) return hipSuccess;
  hipLaunchKernelGGL(robust_tiles_kernel, dim3(n_owned), dim3(PASS_BLOCK), 0, st, reinterpret_cast<const float4*>(chains), reinterpret_cast<float4*>(out),
                     reinterpret_cast<float4*>(tiles), L);
  return hipGetLastError();
}

}  // namespace rene
