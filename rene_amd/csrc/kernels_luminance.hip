// kernels_luminance.hip -- rene_luminance_histogram (include/rene_hip.h): the image-wide statistic automatic exposure needs, in integers.  The
// luminance l = lum3 of every pixel's mean v = s / (float)N_t (N_t == 0: 0) -- the pixels rene_output_tonemapped would write: inside the image,
// and on a tile shard the owned tiles' only -- is counted dark where !(l > 0) and else in one of 256 bins cut from its bit pattern, eight per
// octave from 2^-20 to 2^12: no transcendental, and counts are sums of ones, so the result does not depend on the grid or on the order, and the
// shards' histograms add up to the unsharded one exactly.  Built with ROBUSTFLAGS (Makefile): the division and lum3 are those of the output kernel
// and of the host's rene_luminance_histogram_host.
//
//   A streaming pass: it reads the layer's 16 bytes per pixel and the tiles' divisors as the output kernel does (4 consecutive pixels per thread,
//   straight-line loads from addresses held inside the image) and writes nothing per pixel.  The grid is sized to the chip (the host picks
//   `groups`), and every workgroup strides over the image.  A workgroup counts in LDS, one copy of the histogram per wave (4 x 256 x 4 B): the lanes
//   of a wave that meet in one bin are serialised by the LDS unit, but on a flat image the four waves are not serialised on one word as well.
//   Every workgroup stores its 256 counts and its dark count to its own row of rows[groups][257], and a second launch of one workgroup
//   (1024 threads, four to a column) adds the rows.
//   No global atomics (same-address global atomics run at about 80 M/s on this chip).
#include <hip/hip_runtime.h>

#include "chain_pass.h"
#include "kernels.h"

namespace rene {

namespace {

constexpr uint32_t LUM_WAVES = LUM_BLOCK / 64u, LUM_PIXELS = 4;
static_assert(LUM_BLOCK == LUM_BINS, "thread t clears and stores bin t");

// the bin of a luminance l > 0 (NaN excluded by the caller): bits 30 .. 20 of the pattern are the exponent and three bits of mantissa
__device__ __forceinline__ uint32_t luminance_bin(float l) {
  const int b = (int)(__float_as_uint(l) >> 20) - 856;
  return (uint32_t)min(max(b, 0), (int)LUM_BINS - 1);
}

}  // namespace

__global__ void __launch_bounds__(LUM_BLOCK) luminance_kernel(LuminanceLaunch L) {
  __shared__ uint32_t hist[LUM_WAVES][LUM_BINS];
  __shared__ uint32_t dark_of[LUM_WAVES];
#pragma unroll
  for (uint32_t w = 0; w < LUM_WAVES; ++w) hist[w][threadIdx.x] = 0u;
  if (threadIdx.x < LUM_WAVES) dark_of[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t wave = threadIdx.x / 64u;
  const uint32_t n_px = L.width * L.height;  // (a film has at most 16384 x 16384 pixels: no index below wraps)
  const uint32_t stride = gridDim.x * LUM_BLOCK * LUM_PIXELS;
  const float4* __restrict__ layer = reinterpret_cast<const float4*>(L.layer);
  uint32_t dark = 0u;
  for (uint32_t p0 = (blockIdx.x * LUM_BLOCK + threadIdx.x) * LUM_PIXELS; p0 < n_px; p0 += stride) {
    const uint32_t cnt = min(LUM_PIXELS, n_px - p0);
    uint32_t y = p0 / L.width, x = p0 - y * L.width;
    float4 s[LUM_PIXELS];
    uint32_t n[LUM_PIXELS];
    bool own[LUM_PIXELS];
#pragma unroll
    for (uint32_t j = 0; j < LUM_PIXELS; ++j) {  // (every load is made, as in output_pixels: a pixel past the end or of another shard is read and not counted)
      const uint32_t tile = min((y / RENE_TILE_SIZE) * L.tiles_x + x / RENE_TILE_SIZE, L.n_tiles - 1u);
      uint32_t rem = tile - __umulhi(tile, L.shard_inv) * L.shard_count;
      rem -= rem >= L.shard_count ? L.shard_count : 0u;
      own[j] = j < cnt && (L.shard_count <= 1u || rem == L.shard_rank);
      n[j] = L.tile_frames[tile];
      s[j] = layer[min(p0 + j, n_px - 1u)];
      if (++x == L.width) {
        x = 0u;
        ++y;
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < LUM_PIXELS; ++j) {
      float r = 0.0f, g = 0.0f, b = 0.0f;  // N_t == 0: 0, counted dark
      if (n[j] != 0u) {
        const float d = (float)n[j];
        r = s[j].x / d;
        g = s[j].y / d;
        b = s[j].z / d;
      }
      const float l = lum3(r, g, b);
      if (own[j]) {
        if (l > 0.0f) atomicAdd(&hist[wave][luminance_bin(l)], 1u);
        else ++dark;
      }
    }
  }
  if (dark) atomicAdd(&dark_of[wave], dark);
  __syncthreads();
  uint32_t* __restrict__ row = L.rows + (size_t)blockIdx.x * LUM_ROW;
  uint32_t sum = 0u;
#pragma unroll
  for (uint32_t w = 0; w < LUM_WAVES; ++w) sum += hist[w][threadIdx.x];
  row[threadIdx.x] = sum;
  if (threadIdx.x == 0u) {
    uint32_t d = 0u;
#pragma unroll
    for (uint32_t w = 0; w < LUM_WAVES; ++w) d += dark_of[w];
    row[LUM_BINS] = d;
  }
}

// rows[groups][257] -> out[257], one workgroup of LUM_SUM_PARTS x 256 threads: part p adds the rows p, p + LUM_SUM_PARTS, ... of its column (a serial
// loop over a thousand rows in 256 threads took 0.37 ms, loads one behind the other), the parts meet in LDS
constexpr uint32_t LUM_SUM_PARTS = 4;
__global__ void __launch_bounds__(LUM_SUM_PARTS* LUM_BLOCK) luminance_sum_kernel(const uint32_t* __restrict__ rows, uint32_t groups, uint32_t* __restrict__ out) {
  __shared__ uint32_t partial[LUM_SUM_PARTS][LUM_ROW];
  const uint32_t part = threadIdx.x / LUM_BLOCK, bin = threadIdx.x % LUM_BLOCK;
  for (uint32_t col = bin; col < LUM_ROW; col += LUM_BLOCK) {  // (thread 0 of a part takes the dark count's column as well)
    uint32_t sum = 0u;
#pragma unroll 8
    for (uint32_t g = part; g < groups; g += LUM_SUM_PARTS) sum += rows[(size_t)g * LUM_ROW + col];
    partial[part][col] = sum;
  }
  __syncthreads();
  for (uint32_t col = threadIdx.x; col < LUM_ROW; col += LUM_SUM_PARTS * LUM_BLOCK) {
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t q = 0; q < LUM_SUM_PARTS; ++q) sum += partial[q][col];
    out[col] = sum;
  }
}

hipError_t launch_luminance(const LuminanceLaunch& L, hipStream_t st) {
  if (L.groups == 0u || (size_t)L.width * L.height == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(luminance_kernel, dim3(L.groups), dim3(LUM_BLOCK), 0, st, L);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(luminance_sum_kernel, dim3(1), dim3(LUM_SUM_PARTS * LUM_BLOCK), 0, st, static_cast<const uint32_t*>(L.rows), L.groups, L.out);
  return hipGetLastError();
}

}  // namespace rene
