// output_pixel.h -- the device code the two units of the output transform share: kernels_output.hip (rene_output_8bit: the mean's byte) and
// kernels_tonemap.hip (rene_output_tonemapped: exposure and a tone curve between the mean and its byte).  Both are built with ROBUSTFLAGS
// (Makefile): IEEE division, denormals kept, no contraction -- every operation below is the one include/rene_hip.h names, rounded once.
//
//   The mean is v = s / (float)N_t, the correctly rounded division of tile_mean_kernel (kernels_mean.hip); N_t == 0 gives 0.
//
//   sRGB without a pow that agrees with the host's: rene_to_rgb8 as a map float -> byte is monotone with exactly 255 steps, so the byte is the
//   number of thresholds T[k] <= v, T[k] the smallest float the HOST function maps to k + 1 (rene_output_thresholds derives the table from that
//   function by bisection).  The table, 255 floats, lives in LDS.  An index is guessed from v_log_f32 / v_exp_f32 -- the guess need only be within one
//   step of the truth, and the approximation is within a thousandth of one -- and corrected by two table compares: 6 LDS reads per pixel where an
//   8-step binary search takes 24.  (At HBM rate this kernel moves 19 bytes per pixel, about 2.6 x 10^11 pixels per second: 24 reads per pixel are
//   6 x 10^12 ds_read_b32 lanes per second against 32 conflict-free lanes per clock and CU, 2 x 10^13 per second on the chip -- and the reads of a
//   search go to random banks, several ways conflicted.  6 reads per pixel stay under a tenth of the LDS rate.)  Either way the result is defined
//   by the table, not by the approximation.
//
//   The AOV transforms are one multiply, a clamp and a truncation.
//
//   Mapping: one thread per OUT_PIXELS = 4 consecutive pixels of the image taken as one run of W * H pixels, so a thread's bytes start on a dword
//   of the (4-byte aligned) destination whatever the width: 64 bytes in, 12 or 16 out, consecutive lanes to consecutive bytes, in dwords where all
//   four pixels are written.  On a tile shard only the pixels of owned tiles are written -- a thread whose run crosses into a tile of another
//   shard, and the image's last thread, store their pixels byte by byte (RGB8) or pixel by pixel (RGBA8); every other byte of the destination is
//   left as it was.  No atomics.  Nothing here writes the accumulation state.
//   (RENE_OUT_BLOCK, RENE_OUT_PIXELS: the shape for A/B builds, `make variant EXTRA=-D...`; DESIGN.md section 4c has what 512, 1024 and 8 gave.)
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "chain_pass.h"
#include "kernels.h"

namespace rene {

#ifndef RENE_OUT_BLOCK
#define RENE_OUT_BLOCK 256
#endif
#ifndef RENE_OUT_PIXELS
#define RENE_OUT_PIXELS 4
#endif
constexpr uint32_t OUT_BLOCK = RENE_OUT_BLOCK, OUT_PIXELS = RENE_OUT_PIXELS;
static_assert(OUT_BLOCK >= 256 && OUT_PIXELS % 4 == 0, "the table is loaded by 256 threads; a thread's bytes start on a dword");
constexpr int TONEMAP_NONE = -1;  // output_pixels' OP for rene_output_8bit: the mean goes to its byte as it is

// Rust's `as u8` (rene_hip.cpp, sat_u8): saturating, NaN -> 0
__device__ __forceinline__ uint32_t sat_u8(float v) {
  if (!(v > 0.0f)) return 0u;
  if (v >= 255.0f) return 255u;
  return (uint32_t)v;
}

// one channel: the mean v -> its byte.  `thr`: the thresholds (LDS in the kernel; OUTPUT_SRGB only), padded to 256 entries
template <int TRANSFORM>
__device__ __forceinline__ uint32_t output_byte(float v, const float* thr) {
  if constexpr (TRANSFORM == RENE_OUTPUT_SRGB) {
    v = fmaxf(v, 0.0f);  // NaN and negatives count no threshold, as 0 does
    // the guess: round(255 * gamma(v)) by the hardware's log2 / exp2, within one step of the table's answer; held to 1 .. 254 so that both
    // compares have an entry (+inf: 254, and both compares hold)
    const float p = 1.055f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(v) * (1.0f / 2.4f)) - 0.055f;
    const float g = v <= 0.0031308f ? 12.92f * v : p;
    const uint32_t i = (uint32_t)fminf(fmaxf(255.0f * g + 0.5f, 1.0f), 254.0f);
    return i - 1u + (v >= thr[i - 1u] ? 1u : 0u) + (v >= thr[i] ? 1u : 0u);
  } else {
    if constexpr (TRANSFORM == RENE_OUTPUT_AOV_NORMAL) v = v * 0.5f + 0.5f;  // (two roundings: no contraction in this unit)
    return sat_u8(256.0f * fminf(fmaxf(v, 0.0f), 0.999f));
  }
}

// Exposure and the tone curve of one pixel (include/rene_hip.h, "tone-mapped output"): the mean v -> the value whose sRGB byte is written.
// `w2`: white * white, rounded on the host.  The x86 host's rene_tonemap_rgb8 is the same sequence of fp32 operations.
template <int OP>
__device__ __forceinline__ float3 tonemap_pixel(float3 v, float scale, float w2) {
  if constexpr (OP == TONEMAP_NONE) {
    return v;
  } else {
    static_assert(OP == RENE_TONEMAP_CLAMP || OP == RENE_TONEMAP_REINHARD || OP == RENE_TONEMAP_ACES, "an operator of include/rene_hip.h");
    const float3 e = make_float3(v.x * scale, v.y * scale, v.z * scale);
    if constexpr (OP == RENE_TONEMAP_REINHARD) {
      const float l = fminf(fmaxf(lum3(e.x, e.y, e.z), 0.0f), FLT_MAX);  // (a NaN or negative luminance: 0, and the pixel keeps its values)
      const float q = l / w2;
      const float a = 1.0f + q;
      const float b = 1.0f + l;
      const float f = a / b;
      return make_float3(e.x * f, e.y * f, e.z * f);
    } else if constexpr (OP == RENE_TONEMAP_ACES) {
      auto curve = [](float ec) {
        const float x = fminf(fmaxf(ec, 0.0f), 16777216.0f);
        const float n = x * (2.51f * x + 0.03f);
        const float d = x * (2.43f * x + 0.59f) + 0.14f;
        return n / d;
      };
      return make_float3(curve(e.x), curve(e.y), curve(e.z));
    } else {
      return e;
    }
  }
}

// The table's way into LDS, in two halves so that its latency hides behind loads issued between them: fetch (one global load per thread of the
// first 256) and publish (the LDS write and the barrier)
template <int TRANSFORM>
__device__ __forceinline__ float fetch_threshold(const float* __restrict__ thresholds) {
  if constexpr (TRANSFORM == RENE_OUTPUT_SRGB) return threadIdx.x < 255u ? thresholds[threadIdx.x] : __builtin_inff();
  return 0.0f;
}
template <int TRANSFORM>
__device__ __forceinline__ void publish_threshold(float* lds, float t) {
  if constexpr (TRANSFORM == RENE_OUTPUT_SRGB) {
    if (threadIdx.x < 256u) lds[threadIdx.x] = t;
    __syncthreads();
  }
}

struct alignas(4) Bytes12 {
  uint32_t w[3];
};
struct alignas(4) Bytes16 {
  uint32_t w[4];
};

// The whole of an output kernel: `thr` is the kernel's LDS table (256 floats under RENE_OUTPUT_SRGB).  OP: TONEMAP_NONE, or the operator applied
// between the mean and its byte with `scale` and `w2`.
template <int TRANSFORM, int FORMAT, int OP>
__device__ __forceinline__ void output_pixels(const OutputLaunch& L, float scale, float w2, float* thr) {
  const uint32_t n_px = L.width * L.height;  // (a film has at most 16384 x 16384 pixels)
  const uint32_t p0 = (blockIdx.x * OUT_BLOCK + threadIdx.x) * OUT_PIXELS;
  const uint32_t cnt = p0 < n_px ? min(OUT_PIXELS, n_px - p0) : 0u;
  uint32_t y = p0 / L.width, x = p0 - y * L.width;
  const float t = fetch_threshold<TRANSFORM>(L.thresholds);
  float4 s[OUT_PIXELS];
  uint32_t n[OUT_PIXELS];
  bool wr[OUT_PIXELS];
  const float4* __restrict__ layer = reinterpret_cast<const float4*>(L.layer);
  // the table's load is in flight while the loads of the thread's pixels and of their tiles' frame counts are issued; it is the oldest, so the LDS
  // write and the barrier behind them wait for it alone.  Straight-line code: behind a branch every load would be waited for before the next is
  // issued.  So every load is made, from an address held inside the image and the grid -- a pixel past the image's end or in a tile of another
  // shard is read and not written -- and tile % shard_count is taken without a division: mulhi(tile, floor(2^32 / shard_count)) is the quotient
  // or one less
#pragma unroll
  for (uint32_t j = 0; j < OUT_PIXELS; ++j) {
    const uint32_t tile = min((y / RENE_TILE_SIZE) * L.tiles_x + x / RENE_TILE_SIZE, L.n_tiles - 1u);
    uint32_t rem = tile - __umulhi(tile, L.shard_inv) * L.shard_count;
    rem -= rem >= L.shard_count ? L.shard_count : 0u;
    wr[j] = j < cnt && (L.shard_count <= 1u || rem == L.shard_rank);
    n[j] = L.tile_frames[tile];
    s[j] = layer[min(p0 + j, n_px - 1u)];
    if (++x == L.width) {
      x = 0u;
      ++y;
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // (nothing that consumes a load is scheduled up between the loads: it would wait for them one by one)
  publish_threshold<TRANSFORM>(thr, t);
  if (cnt == 0u) return;  // (the film has pixels: n_px - 1 above is one of them)
  uint32_t px[OUT_PIXELS];
#pragma unroll
  for (uint32_t j = 0; j < OUT_PIXELS; ++j) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // N_t == 0: 0
    if (n[j] != 0u) {
      const float d = (float)n[j];
      v.x = s[j].x / d;
      v.y = s[j].y / d;
      v.z = s[j].z / d;
    }
    if constexpr (OP != TONEMAP_NONE) {
      const float3 c = tonemap_pixel<OP>(make_float3(v.x, v.y, v.z), scale, w2);
      v.x = c.x, v.y = c.y, v.z = c.z;
    }
    px[j] = output_byte<TRANSFORM>(v.x, thr) | output_byte<TRANSFORM>(v.y, thr) << 8 | output_byte<TRANSFORM>(v.z, thr) << 16 | 0xff000000u;
  }
#pragma unroll
  for (uint32_t g = 0; g < OUT_PIXELS; g += 4u) {  // four pixels at a time: 12 or 16 bytes from a dword boundary
    const bool all = wr[g] && wr[g + 1u] && wr[g + 2u] && wr[g + 3u];
    if constexpr (FORMAT == RENE_OUTPUT_RGBA8) {
      uint32_t* dst = static_cast<uint32_t*>(L.dst) + (size_t)p0 + g;
      if (all) {
        *reinterpret_cast<Bytes16*>(dst) = Bytes16{{px[g], px[g + 1u], px[g + 2u], px[g + 3u]}};
      } else {
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
          if (wr[g + j]) dst[j] = px[g + j];
      }
    } else {
      uint8_t* dst = static_cast<uint8_t*>(L.dst) + ((size_t)p0 + g) * 3u;
      if (all) {
        const uint32_t a = px[g] & 0xffffffu, b = px[g + 1u] & 0xffffffu, c = px[g + 2u] & 0xffffffu, d = px[g + 3u] & 0xffffffu;
        *reinterpret_cast<Bytes12*>(dst) = Bytes12{{a | b << 24, b >> 8 | c << 16, c >> 16 | d << 8}};
      } else {
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
          if (wr[g + j]) {
            dst[3u * j] = (uint8_t)px[g + j];
            dst[3u * j + 1u] = (uint8_t)(px[g + j] >> 8);
            dst[3u * j + 2u] = (uint8_t)(px[g + j] >> 16);
          }
      }
    }
  }
}

}  // namespace rene
