// kernels_exr_passes.hip -- the body of a pass-layer OpenEXR file on the device (rene_output_exr_passes, include/rene_hip.h): the records of the
// occlusion, direct-light, bounce and light-group passes and the radiance sums in, the scan-line chunks of an uncompressed file out, in their
// final byte layout -- bit for bit the bytes of the host's rene_exr_passes_body_host.
//
//   The body: row y is one chunk at y * (8 + W * bpp) -- int32 y, int32 W * bpp, then the row of every chosen channel in turn, the channels in the
//   order of their names' bytes (the kernel emits them in that order; it is static, the names of light groups live in an attribute):
//     ao | bent.X .Y .Z | depth0.B .G .R .. depth9.B .G .R | direct.B .G .R | indirect.B .G .R | light0.B .G .R .. light7.B .G .R | pathlength
//   Every channel is HALF: 2 bytes per pixel.
//
//   Mapping: exr_kernel's -- the grid's y is the row and a lane is one pixel of it, so 64 consecutive lanes store 128 consecutive bytes of one
//   channel row, each a naturally aligned 2-byte store.  The only 4-byte values are the row's prefix, which sits at an address = 2 (mod 4) where
//   W * bpp = 2 (mod 4) and y is odd: store_word's two-halves form (exr_store.h).  A tile shard writes the bytes of its own tiles' pixels, and
//   the lane of x = 0 the row's prefix where the shard owns a tile of that tile row.  The layer mask and the group mask are arguments: one
//   kernel, no instantiation per mask.  No LDS, no atomics.  Nothing here writes the records, the accumulation state or the denoiser's buffers.
//
//   Loads: with every layer a lane reads 416 bytes, 104 dwords -- exr_kernel's "every load ahead of the first conversion" would hold them all
//   at once.  Here the loads are grouped per source record, in file order, and each group is issued ahead of its own conversions: the occlusion
//   record (8 dwords), the bounce record (44), the direct record and the radiance sum (16), the chosen groups of the light record (up to 33:
//   eight 16-byte groups and n).  pathlength, the last row, keeps the bounce record's n and length_sum in two registers until then.
//
// The specification fixes every fp32 operation: this unit is built with ROBUSTFLAGS (Makefile) -- the correctly rounded division and square root,
// denormals kept, no contraction -- and the halves follow half_element.h's rule, with every NaN written as 0x7e00.
#include <hip/hip_runtime.h>

#include "exr_store.h"
#include "half_element.h"
#include "kernels.h"

namespace rene {

constexpr uint32_t EXR_PASSES_BLOCK = 256;

namespace {

__device__ __forceinline__ float mean_of(float s, float n_f, bool any) { return any ? s / n_f : 0.0f; }
__device__ __forceinline__ float f(uint32_t bits) { return __uint_as_float(bits); }

}  // namespace

__global__ void __launch_bounds__(EXR_PASSES_BLOCK) exr_passes_kernel(ExrPassesLaunch L) {
  const uint32_t y = blockIdx.y, x = blockIdx.x * EXR_PASSES_BLOCK + threadIdx.x;
  if (x >= L.width) return;
  const uint32_t F = L.layers;
  const uint32_t row_data = L.width * L.bytes_per_pixel;  // (at most 16384 x 130)
  const size_t row_at = (size_t)y * (8u + (size_t)row_data);
  uint8_t* const row = static_cast<uint8_t*>(L.dst) + row_at;
  const uint32_t row_lo = (uint32_t)row_at;  // (the destination is 4-byte aligned: the prefix's alignment follows from these low bits)
  const uint32_t tile = (y / RENE_TILE_SIZE) * L.tiles_x + x / RENE_TILE_SIZE;
  bool prefix = x == 0u;
  if (L.shard_count > 1u) {
    if (prefix) {  // does the shard own one of the tiles tile .. tile + tiles_x - 1 of this tile row?
      const uint32_t first = tile % L.shard_count;
      const uint32_t d = (L.shard_rank + L.shard_count - first) % L.shard_count;
      prefix = d < L.tiles_x;
    }
    uint32_t rem = tile - __umulhi(tile, L.shard_inv) * L.shard_count;  // mulhi(tile, floor(2^32 / shard_count)) is the quotient or one less
    rem -= rem >= L.shard_count ? L.shard_count : 0u;
    if (prefix) {
      store_word(row, y, (row_lo & 2u) == 0u);
      store_word(row + 4, row_data, (row_lo & 2u) == 0u);
    }
    if (rem != L.shard_rank) return;
  } else if (prefix) {
    store_word(row, y, (row_lo & 2u) == 0u);
    store_word(row + 4, row_data, (row_lo & 2u) == 0u);
  }
  const size_t p = (size_t)y * L.width + x;
  uint32_t off = 8u + 2u * x;  // this lane's place in the next channel row of the chunk
  auto channel = [&](float v) {
    const _Float16 h = to_element<_Float16>(v);
    *reinterpret_cast<uint16_t*>(row + off) = v != v ? (uint16_t)0x7e00u : __builtin_bit_cast(uint16_t, h);
    off += 2u * L.width;
  };
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  // ao | bent.X .Y .Z: the occlusion record {hits, rays, occluded, n} {bent_sum, reserved}
  if (F & (RENE_EXRP_AO | RENE_EXRP_BENT)) {
    const uint4* rec = reinterpret_cast<const uint4*>(L.occlusion) + 2u * p;
    uint4 o0 = zero, o1 = zero;
    if (F & RENE_EXRP_AO) o0 = rec[0];
    if (F & RENE_EXRP_BENT) o1 = rec[1];
    __builtin_amdgcn_sched_barrier(0);  // (nothing that consumes a load is scheduled up between the loads: it would wait for them one by one)
    if (F & RENE_EXRP_AO) channel(o0.y ? 1.0f - (float)o0.z / (float)o0.y : 1.0f);
    if (F & RENE_EXRP_BENT) {
      const float bx = f(o1.x), by = f(o1.y), bz = f(o1.z);
      const float l = __fsqrt_rn((bx * bx + by * by) + bz * bz);
      const bool some = l > 0.0f;  // (false for a NaN)
      channel(some ? bx / l : 0.0f);
      channel(some ? by / l : 0.0f);
      channel(some ? bz / l : 0.0f);
    }
  }

  // depth0.B .G .R .. depth9.B .G .R: the bounce record, ten {sum, reached} and {n, length_sum, length_max, capped}
  uint32_t bounce_n = 0u, length_sum = 0u;
  if (F & (RENE_EXRP_BOUNCES | RENE_EXRP_LENGTH)) {
    const uint4* rec = reinterpret_cast<const uint4*>(L.bounces) + 11u * p;
    uint4 b[RENE_BOUNCES_BUCKETS];
#pragma unroll
    for (uint32_t d = 0; d < RENE_BOUNCES_BUCKETS; ++d) b[d] = zero;
    if (F & RENE_EXRP_BOUNCES) {
#pragma unroll
      for (uint32_t d = 0; d < RENE_BOUNCES_BUCKETS; ++d) b[d] = rec[d];
    }
    const uint4 tail = rec[RENE_BOUNCES_BUCKETS];
    __builtin_amdgcn_sched_barrier(0);
    bounce_n = tail.x, length_sum = tail.y;
    if (F & RENE_EXRP_BOUNCES) {
      const float n_f = (float)bounce_n;
#pragma unroll
      for (uint32_t d = 0; d < RENE_BOUNCES_BUCKETS; ++d) {
        channel(mean_of(f(b[d].z), n_f, bounce_n != 0u));
        channel(mean_of(f(b[d].y), n_f, bounce_n != 0u));
        channel(mean_of(f(b[d].x), n_f, bounce_n != 0u));
      }
    }
  }

  // direct.B .G .R | indirect.B .G .R: the direct record {seen, hits} {distant, n} {sampled, reserved} and the radiance sum
  if (F & (RENE_EXRP_DIRECT | RENE_EXRP_INDIRECT)) {
    const uint4* rec = reinterpret_cast<const uint4*>(L.direct) + 3u * p;
    const uint4 d0 = rec[0], d1 = rec[1], d2 = rec[2];
    float4 bty = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (F & RENE_EXRP_INDIRECT) bty = reinterpret_cast<const float4*>(L.beauty)[p];
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t n = d1.w;
    const float n_f = (float)n;
    const float sr = (f(d0.x) + f(d1.x)) + f(d2.x), sg = (f(d0.y) + f(d1.y)) + f(d2.y), sb = (f(d0.z) + f(d1.z)) + f(d2.z);
    if (F & RENE_EXRP_DIRECT) {
      channel(mean_of(sb, n_f, n != 0u));
      channel(mean_of(sg, n_f, n != 0u));
      channel(mean_of(sr, n_f, n != 0u));
    }
    if (F & RENE_EXRP_INDIRECT) {
      channel(mean_of(bty.z - sb, n_f, n != 0u));
      channel(mean_of(bty.y - sg, n_f, n != 0u));
      channel(mean_of(bty.x - sr, n_f, n != 0u));
    }
  }

  // light0.B .G .R .. light7.B .G .R, the groups of the mask: the light record, eight {sum, adds} and {n, lit, reserved}
  if (F & RENE_EXRP_LIGHTS) {
    const uint4* rec = reinterpret_cast<const uint4*>(L.lights) + 9u * p;
    uint4 g[RENE_LIGHTS_GROUPS];
#pragma unroll
    for (uint32_t k = 0; k < RENE_LIGHTS_GROUPS; ++k) {
      g[k] = zero;
      if (L.groups >> k & 1u) g[k] = rec[k];
    }
    const uint32_t n = reinterpret_cast<const uint32_t*>(rec + RENE_LIGHTS_GROUPS)[0];
    __builtin_amdgcn_sched_barrier(0);
    const float n_f = (float)n;
#pragma unroll
    for (uint32_t k = 0; k < RENE_LIGHTS_GROUPS; ++k) {
      if (!(L.groups >> k & 1u)) continue;
      channel(mean_of(f(g[k].z), n_f, n != 0u));
      channel(mean_of(f(g[k].y), n_f, n != 0u));
      channel(mean_of(f(g[k].x), n_f, n != 0u));
    }
  }

  if (F & RENE_EXRP_LENGTH) channel(mean_of((float)length_sum, (float)bounce_n, bounce_n != 0u));  // pathlength
}

hipError_t launch_exr_passes(const ExrPassesLaunch& L, hipStream_t st) {
  if (L.width == 0 || L.height == 0) return hipSuccess;
  if (L.height > 65535u || L.bytes_per_pixel < 2u || L.bytes_per_pixel > 130u || (L.layers & ~RENE_EXRP_ALL) || L.groups > 255u) return hipErrorInvalidValue;
  if (((L.layers & RENE_EXRP_LIGHTS) != 0u) != (L.groups != 0u)) return hipErrorInvalidValue;
  // the chunk the kernel walks is the chunk the caller sized: a row per chosen channel
  const uint32_t F = L.layers;
  const uint32_t rows = (F & RENE_EXRP_AO ? 1u : 0u) + (F & RENE_EXRP_BENT ? 3u : 0u) + (F & RENE_EXRP_BOUNCES ? 30u : 0u) + (F & RENE_EXRP_DIRECT ? 3u : 0u) +
                        (F & RENE_EXRP_INDIRECT ? 3u : 0u) + 3u * (uint32_t)__builtin_popcount(L.groups) + (F & RENE_EXRP_LENGTH ? 1u : 0u);
  if (2u * rows != L.bytes_per_pixel) return hipErrorInvalidValue;
  if (((F & (RENE_EXRP_AO | RENE_EXRP_BENT)) && !L.occlusion) || ((F & (RENE_EXRP_BOUNCES | RENE_EXRP_LENGTH)) && !L.bounces) ||
      ((F & (RENE_EXRP_DIRECT | RENE_EXRP_INDIRECT)) && !L.direct) || ((F & RENE_EXRP_LIGHTS) && !L.lights) || ((F & RENE_EXRP_INDIRECT) && !L.beauty) || !L.dst)
    return hipErrorInvalidValue;
  const dim3 grid((L.width + EXR_PASSES_BLOCK - 1u) / EXR_PASSES_BLOCK, L.height), block(EXR_PASSES_BLOCK);
  hipLaunchKernelGGL(exr_passes_kernel, grid, block, 0, st, L);
  return hipGetLastError();
}

}  // namespace rene
