// kernels_denoise_shard.hip -- the `atrous` denoiser on tile shards (rene_denoise_shard_prepare, rene_denoise_place_shard; include/rene_hip.h).  Only
// prepare reads the frame chains, and it is strictly per pixel; the passes and finalize read nothing but the records prepare wrote.  So every shard
// prepares the tiles it owns into a tile-packed buffer, the buffers travel to one context, and that context runs the masked passes and finalize of
// kernels_denoise_tiles.hip on the assembled records, unchanged.  No halo is exchanged and no pixel's arithmetic differs from rene_denoise_tiles'.
//
//   prepare   denoise_shard_prepare_kernel: the text of denoise_tiles_prepare_kernel (atrous_kernels.inc, ATROUS_TILES 1) with ATROUS_PACKED 1 -- the
//             same loads, the same arithmetic, the same validity and (float)N_t in the second guide record; the stores land in the owned tile's
//             block (kernels.h, DN_PACKED_*), and a slot outside the image is stored as zeros: the buffer is deterministic byte for byte
//   place     denoise_shard_place_kernel: one workgroup per packed tile, thread j takes slots j, j + 256, j + 512, j + 768 (consecutive lanes read
//             consecutive 16-byte records) and moves them to the pixel chain_pass.h's slot -> pixel map names.  Moves only: the bits arrive as sent
//
// A unit of its own: the kernels of the two other units stay instruction for instruction what they are.  No atomics, no LDS.
#include <hip/hip_runtime.h>

#include "atrous_filter.h"

namespace rene {

#define ATROUS_TILES 1
#define ATROUS_PACKED 1
#include "atrous_kernels.inc"
#undef ATROUS_TILES

__global__ void __launch_bounds__(PASS_BLOCK) denoise_shard_place_kernel(const float4* __restrict__ body, float4* __restrict__ rec, float4* __restrict__ guides,
                                                                        float* __restrict__ var_plane, TileGrid G) {
  const uint32_t tile = G.shard_rank + blockIdx.x * G.shard_count;
  const uint32_t tiles_y = (G.height + RENE_TILE_SIZE - 1u) / RENE_TILE_SIZE;
  if (tile >= G.tiles_x * tiles_y) return;  // (the host launches one workgroup per tile the rank owns: never taken)
  const uint2 o = image_tile_origin(G, tile);
  const float4* block = body + (size_t)blockIdx.x * DN_PACKED_TILE_F4;
  const float* block_var = reinterpret_cast<const float*>(block + DN_PACKED_VAR_F4);
#pragma unroll
  for (uint32_t q = 0; q < PASS_PER_THREAD; ++q) {
    const uint32_t r = threadIdx.x + q * PASS_BLOCK;
    const uint2 d = slot_pixel(r);
    const uint32_t x = o.x + d.x, y = o.y + d.y;
    if (x >= G.width || y >= G.height) continue;
    const size_t p = (size_t)y * G.width + x;
    rec[p] = block[r];
    guides[2 * p] = block[DN_PACKED_GUIDES_F4 + 2u * r];
    guides[2 * p + 1] = block[DN_PACKED_GUIDES_F4 + 2u * r + 1u];
    var_plane[p] = block_var[r];
  }
}

hipError_t launch_denoise_shard_prepare(const float* chains, const float* image, void* body, const DenoiseLaunch& D, const DenoiseTileSets& T, hipStream_t st) {
  static_assert(TILE_SLOTS % DN_PREPARE_BLOCK == 0, "a prepare workgroup lies inside one tile");
  static_assert(DN_PACKED_TILE_BYTES == 52u * TILE_SLOTS, "52 bytes per slot");
  if (D.grid.n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_shard_prepare_kernel, dim3((D.grid.n_slots + DN_PREPARE_BLOCK - 1u) / DN_PREPARE_BLOCK), dim3(DN_PREPARE_BLOCK), 0, st,
                     reinterpret_cast<const float4*>(chains), reinterpret_cast<const float4*>(image), static_cast<float4*>(body), static_cast<float4*>(body),
                     static_cast<float*>(body), D, T);
  return hipGetLastError();
}

hipError_t launch_denoise_shard_place(const void* body, uint32_t n_owned, float* rec, float* guides, float* var_plane, const TileGrid& G, hipStream_t st) {
  if (n_owned == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_shard_place_kernel, dim3(n_owned), dim3(PASS_BLOCK), 0, st, static_cast<const float4*>(body), reinterpret_cast<float4*>(rec),
                     reinterpret_cast<float4*>(guides), var_plane, G);
  return hipGetLastError();
}

}  // namespace rene
