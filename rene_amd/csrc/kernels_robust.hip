// kernels_robust.hip -- the firefly-robust resolve (rene_resolve_robust, include/rene_hip.h): per owned pixel the trimmed mean over the eight frame
// chains (device_scene.h, CHAINS), how many chains are trimmed following from the Gini coefficient of the chains' luminances; per owned 32 x 32
// tile the sums of the plain and of the robust mean's luminance, so that the caller sees what the trimming removed.
//
//   one workgroup of 256 threads per OWNED tile k, as in kernels_noise.hip (image tile shard_rank + k * shard_count; thread j takes slots j,
//   j + 256, j + 512, j + 768 of the tile's 1024 contiguous slots and reads layer 0 of all eight chains for them: 32 independent 16-byte loads
//   per thread, all issued before the first is waited for); each thread writes one 16-byte vector store per pixel, {rgb, (float)j}, into the
//   pixel-major [H][W][4] output.
//
// The specification fixes every fp32 operation and its order, so this unit is compiled with -ffp-contract=off (no fused multiply-add is formed)
// and, like kernels_mean.hip, without the two options that trade the correctly rounded division and the denormals for speed (Makefile,
// ROBUSTFLAGS): the pixels are bit for bit the numpy restatement's (tests/robust_reference.py), and where nothing is trimmed rene_download_mean's.
//
// The tile sums are reduced in a FIXED order -- a thread's four slots in slot order, a butterfly over the wave's 64 lanes, the four wave partials
// through LDS added in wave order by one lane -- and stored with one 16-byte vector store per tile: no atomics.
//
// Adaptive sampling: where the owned tiles differ in their frame counts the host hands over the chain counts n_c of every distinct N_t and a set
// index per owned tile (RobustLaunch::sets, ::tile_set); the kernel replaces its counts by the tile's before the arithmetic.
//
// Nothing here writes the accumulation state.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rene {

namespace {

constexpr uint32_t ROBUST_BLOCK = 256, ROBUST_PER_THREAD = TILE_SLOTS / ROBUST_BLOCK, ROBUST_WAVES = ROBUST_BLOCK / 64;

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

}  // namespace

__global__ void __launch_bounds__(ROBUST_BLOCK) robust_tiles_kernel(const float4* __restrict__ chains, float4* __restrict__ out, float4* __restrict__ tiles, RobustLaunch L) {
  __shared__ float s_plain[ROBUST_WAVES], s_robust[ROBUST_WAVES];
  __shared__ uint32_t s_n[ROBUST_WAVES], s_trim[ROBUST_WAVES];
  const uint32_t k = blockIdx.x;  // owned tile (the grid is exactly the owned tiles: k * 1024 + 1023 < n_slots)
  if (L.tile_set != nullptr) {    // per-tile chain counts (workgroup-uniform: scalar loads)
    const uint32_t* c = L.sets + (size_t)L.tile_set[k] * CHAINS;
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) L.chain_n[g] = c[g];
  }
  uint32_t n_total = 0, kk = 0;  // N_t and the chains that have received frames
  float nf[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    n_total += L.chain_n[g];
    kk += L.chain_n[g] ? 1u : 0u;
    nf[g] = (float)L.chain_n[g];
  }
  const uint32_t j_cap = kk ? min(L.max_trim, (kk - 1u) / 2u) : 0u;
  const float kf = (float)kk, half_k = kf * 0.5f, n_total_f = (float)n_total;
  const uint32_t tile = L.shard_rank + k * L.shard_count;
  const uint32_t x0 = (tile % L.tiles_x) * RENE_TILE_SIZE, y0 = (tile / L.tiles_x) * RENE_TILE_SIZE;
  const size_t n4 = (size_t)3 * L.n_slots, base = (size_t)k * TILE_SLOTS + threadIdx.x;
  float4 c[ROBUST_PER_THREAD][CHAINS];
#pragma unroll
  for (uint32_t q = 0; q < ROBUST_PER_THREAD; ++q)
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) c[q][g] = chains[(size_t)g * n4 + base + q * ROBUST_BLOCK];  // layer 0 of chain g
  float a = 0.0f, b = 0.0f;
  uint32_t n = 0, n_trim = 0;
#pragma unroll
  for (uint32_t q = 0; q < ROBUST_PER_THREAD; ++q) {
    const uint32_t r = threadIdx.x + q * ROBUST_BLOCK, sub = r >> 6, l = r & 63u;
    const uint32_t x = x0 + (sub & 3u) * 8u + (l & 7u), y = y0 + (sub >> 2) * 8u + (l >> 3);
    if (x >= L.width || y >= L.height) continue;  // a ragged tile's slots outside the image: nothing is written, nothing counted
    float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float lum_plain = 0.0f, lum_robust = 0.0f;
    if (n_total != 0) {
      // steps 1 to 3: the chains' luminances, their ranks, the Gini coefficient
      float lc[CHAINS];
#pragma unroll
      for (uint32_t g = 0; g < CHAINS; ++g) lc[g] = L.chain_n[g] ? lum3(c[q][g].x / nf[g], c[q][g].y / nf[g], c[q][g].z / nf[g]) : 0.0f;
      uint32_t rank[CHAINS];
      float tot = 0.0f, num = 0.0f;
#pragma unroll
      for (uint32_t g = 0; g < CHAINS; ++g) {
        rank[g] = 0;
        if (!L.chain_n[g]) continue;
#pragma unroll
        for (uint32_t h = 0; h < CHAINS; ++h) {
          if (h == g || !L.chain_n[h]) continue;
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
        const bool kept = !L.chain_n[g] || (rank[g] >= j && rank[g] < kk - j);
        if (kept) {
          ar += c[q][g].x;
          ag += c[q][g].y;
          ab += c[q][g].z;
          n_kept += L.chain_n[g];
        }
      }
      const float nk = (float)n_kept;  // j <= (k - 1) / 2: at least one non-empty chain is kept
      res = make_float4(ar / nk, ag / nk, ab / nk, (float)j);
      lum_robust = lum3(res.x, res.y, res.z);
      lum_plain = lum3(sr / n_total_f, sg / n_total_f, sb / n_total_f);
      n_trim += j ? 1u : 0u;
    }
    out[(size_t)y * L.width + x] = res;  // one 16-byte vector store per pixel
    a += lum_plain;
    b += lum_robust;
    n += 1u;
  }
  a = wave_sum(a);
  b = wave_sum(b);
  n = wave_sum(n);
  n_trim = wave_sum(n_trim);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
    s_plain[wave] = a;
    s_robust[wave] = b;
    s_n[wave] = n;
    s_trim[wave] = n_trim;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = s_plain[0], tb = s_robust[0];
    uint32_t tn = s_n[0], tt = s_trim[0];
#pragma unroll
    for (uint32_t w = 1; w < ROBUST_WAVES; ++w) {
      ta += s_plain[w];
      tb += s_robust[w];
      tn += s_n[w];
      tt += s_trim[w];
    }
    tiles[k] = make_float4(ta, tb, __uint_as_float(tn), __uint_as_float(tt));  // one 16-byte vector store per tile
  }
}

hipError_t launch_robust_tiles(const float* chains, float* out, float* tiles, const RobustLaunch& L, hipStream_t st) {
  const uint32_t n_owned = L.n_slots / TILE_SLOTS;
  if (n_owned == 0) return hipSuccess;
  hipLaunchKernelGGL(robust_tiles_kernel, dim3(n_owned), dim3(ROBUST_BLOCK), 0, st, reinterpret_cast<const float4*>(chains), reinterpret_cast<float4*>(out),
                     reinterpret_cast<float4*>(tiles), L);
  return hipGetLastError();
}

}  // namespace rene
