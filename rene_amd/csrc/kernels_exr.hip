// kernels_exr.hip -- the body of a multi-channel OpenEXR file on the device (rene_output_exr, include/rene_hip.h): the sums of up to three image
// layers, the denoised or robust record, the geometry pass's 64-byte record and the tile's N_t in, the scan-line chunks of an uncompressed file out,
// in their final byte layout -- bit for bit the bytes of the host's rene_exr_body_host.
//
//   The body: row y is one chunk at y * (8 + W * bpp) -- int32 y, int32 W * bpp, then the row of every chosen channel in turn, the channels in the
//   order of their names' bytes (the table of rene_hip.cpp, kExrChannels; the kernel emits them in the same order):
//     A | B G | P.X P.Y P.Z | R | Z | albedo.B .G .R | cov0 .. cov3 | denoised.B .G .R | id0 .. id3 | normal.X .Y .Z
//   HALF channels are 2 bytes per pixel, FLOAT and UINT channels 4.
//
//   Mapping: the grid's y is the row and a lane is one pixel of it, so 64 consecutive lanes store 64 consecutive values of one channel row: a
//   HALF leaves as a 2-byte store (a wave: 128 consecutive bytes), a FLOAT or UINT as a dword (256).  (A lane per pixel pair, with the two halves
//   in one dword, was built first and measured against this shape at 1920 x 1080: equal with BEAUTY alone, 1.38 times slower with every layer --
//   68 VGPRs and twice the loads in flight per lane against 42; profiles/exr_shape_ab.jsonl)
//   Every store is naturally aligned.  A channel row starts on an even byte; where a 4-byte channel's row, or a row's prefix, starts at an
//   address = 2 (mod 4) -- odd W only, and the same for every lane of the row -- the value leaves as two 16-bit stores (store_word: through a
//   volatile access, because the backend otherwise joins the two into the one unaligned dword store this target would let it issue).
//   A tile shard writes the bytes of its own tiles' pixels, and the lane of x = 0 the row's prefix where the shard owns a tile of that tile row.
//   Every load is issued before the first value is converted; no LDS, no atomics.  Nothing here writes the accumulation state, the denoiser's
//   buffers or the records.
//
// The specification fixes every fp32 operation: this unit is built with ROBUSTFLAGS (Makefile) -- the correctly rounded division, denormals kept, no
// contraction -- and the halves follow half_element.h's rule, which it shares with kernels_features.hip.
#include <hip/hip_runtime.h>

#include "exr_store.h"
#include "half_element.h"
#include "kernels.h"

namespace rene {

constexpr uint32_t EXR_BLOCK = 256;

namespace {

__device__ __forceinline__ float mean_of(float s, uint32_t n) { return n ? s / (float)n : 0.0f; }
}  // namespace

__global__ void __launch_bounds__(EXR_BLOCK) exr_kernel(ExrLaunch L) {
  const uint32_t y = blockIdx.y, x = blockIdx.x * EXR_BLOCK + threadIdx.x;
  if (x >= L.width) return;
  const uint32_t F = L.layers;
  const uint32_t row_data = L.width * L.bytes_per_pixel;  // (at most 16384 x 66)
  const size_t row_at = (size_t)y * (8u + (size_t)row_data);
  uint8_t* const row = static_cast<uint8_t*>(L.dst) + row_at;
  const uint32_t row_lo = (uint32_t)row_at;  // (the destination is 4-byte aligned: the alignment of a channel row follows from these low bits)
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
  // the loads, all of them ahead of the first use
  const size_t p = (size_t)y * L.width + x;
  float4 bty = make_float4(0.0f, 0.0f, 0.0f, 0.0f), alb = bty, nrm = bty, dno = bty;
  uint4 g0 = make_uint4(0u, 0u, 0u, 0u), g1 = g0, g2 = g0, g3 = g0;
  uint32_t n_bty = 0u, n_img = 0u, n_dno = 0u;
  if (F & RENE_EXR_BEAUTY) n_bty = L.beauty_frames[tile], bty = reinterpret_cast<const float4*>(L.beauty)[p];
  if (F & (RENE_EXR_ALBEDO | RENE_EXR_NORMAL)) n_img = L.image_frames[tile];
  if (F & RENE_EXR_ALBEDO) alb = reinterpret_cast<const float4*>(L.albedo)[p];
  if (F & RENE_EXR_NORMAL) nrm = reinterpret_cast<const float4*>(L.normal)[p];
  if (F & RENE_EXR_DENOISED) n_dno = L.denoised_frames[tile], dno = reinterpret_cast<const float4*>(L.denoised)[p];
  const uint4* rec = reinterpret_cast<const uint4*>(L.records) + 4u * p;  // {depth_sum, depth_min, hits, n} {position_sum, other} {id} {count}
  if (F & (RENE_EXR_ALPHA | RENE_EXR_DEPTH | RENE_EXR_POSITION | RENE_EXR_IDS)) g0 = rec[0];
  if (F & RENE_EXR_POSITION) g1 = rec[1];
  if (F & RENE_EXR_IDS) g2 = rec[2], g3 = rec[3];
  __builtin_amdgcn_sched_barrier(0);  // (nothing that consumes a load is scheduled up between the loads: it would wait for them one by one)

  uint32_t off = 8u;  // the next channel row's offset in the chunk
  auto half_channel = [&](float v) {
    *reinterpret_cast<_Float16*>(row + off + 2u * x) = to_element<_Float16>(v);
    off += 2u * L.width;
  };
  auto word_channel = [&](uint32_t bits) {  // a FLOAT or UINT channel
    store_word(row + off + 4u * x, bits, ((row_lo + off) & 2u) == 0u);
    off += 4u * L.width;
  };
  const uint32_t hits = g0.z, n = g0.w;
  const float hits_f = (float)hits, n_f = (float)n;
  // the channels in the order of their names (capitals, then lower case)
  if (F & RENE_EXR_ALPHA) half_channel(n ? hits_f / n_f : 0.0f);  // A
  if (F & RENE_EXR_BEAUTY) {
    half_channel(mean_of(bty.z, n_bty));  // B
    half_channel(mean_of(bty.y, n_bty));  // G
  }
  if (F & RENE_EXR_POSITION) {  // P.X P.Y P.Z = position_sum / hits, 0 where nothing hit
    word_channel(__float_as_uint(hits ? __uint_as_float(g1.x) / hits_f : 0.0f));
    word_channel(__float_as_uint(hits ? __uint_as_float(g1.y) / hits_f : 0.0f));
    word_channel(__float_as_uint(hits ? __uint_as_float(g1.z) / hits_f : 0.0f));
  }
  if (F & RENE_EXR_BEAUTY) half_channel(mean_of(bty.x, n_bty));  // R
  if (F & RENE_EXR_DEPTH) word_channel(__float_as_uint(hits ? __uint_as_float(g0.x) / hits_f : __builtin_inff()));  // Z = depth_sum / hits
  if (F & RENE_EXR_ALBEDO) {
    half_channel(mean_of(alb.z, n_img));
    half_channel(mean_of(alb.y, n_img));
    half_channel(mean_of(alb.x, n_img));
  }
  if (F & RENE_EXR_IDS) {  // cov k = count[k] / n
    half_channel(n ? (float)g3.x / n_f : 0.0f);
    half_channel(n ? (float)g3.y / n_f : 0.0f);
    half_channel(n ? (float)g3.z / n_f : 0.0f);
    half_channel(n ? (float)g3.w / n_f : 0.0f);
  }
  if (F & RENE_EXR_DENOISED) {
    half_channel(mean_of(dno.z, n_dno));
    half_channel(mean_of(dno.y, n_dno));
    half_channel(mean_of(dno.x, n_dno));
  }
  if (F & RENE_EXR_IDS) {
    word_channel(g2.x);
    word_channel(g2.y);
    word_channel(g2.z);
    word_channel(g2.w);
  }
  if (F & RENE_EXR_NORMAL) {
    half_channel(mean_of(nrm.x, n_img));
    half_channel(mean_of(nrm.y, n_img));
    half_channel(mean_of(nrm.z, n_img));
  }
}

hipError_t launch_exr(const ExrLaunch& L, hipStream_t st) {
  if (L.width == 0 || L.height == 0) return hipSuccess;
  if (L.height > 65535u || L.bytes_per_pixel == 0u) return hipErrorInvalidValue;
  const dim3 grid((L.width + EXR_BLOCK - 1u) / EXR_BLOCK, L.height), block(EXR_BLOCK);
  hipLaunchKernelGGL(exr_kernel, grid, block, 0, st, L);
  return hipGetLastError();
}

}  // namespace rene
