// pixel_pass.h -- what the per-pixel frame-range passes share on the device and at the launch: the geometry pass (kernels_gbuffer.hip), the occlusion
// pass (kernels_occlusion.hip), the direct-light pass (kernels_direct.hip), the bounce pass (kernels_bounces.hip) and the light-group pass
// (kernels_lights.hip), each with its per-sample probe.  Included behind device_code.inc, inside namespace rene.
//
// The family: one lane per pixel slot of an owned tile, through the slot -> pixel map of the chain passes in item_slot.h's spelling (slot_x /
// slot_yi), so a wave is an 8 x 8 micro-tile of coherent rays and a tile shard covers exactly its tiles.  A lane loops over a range of frames
// in frame order -- the frame's seed from a device array the host filled with rene_frame_seeds (a wave-uniform index: a scalar load), the primary
// ray (primary_ray.h) -- keeps its sums on chip (in registers; the bounce pass's bucket words and the light-group pass's sample in an LDS column
// of the lane's own) and stores its finished record in 16-byte pieces.  A slot outside the image keeps its wave converged on a clamped pixel and stores nothing; the host zeroes
// the destination, so the pixels of tiles the context does not own are the all-zero record.  No atomics, and nothing of the context is written
// but the destination.
#pragma once

// the calling lane's pixel: slot blockIdx.x * BLOCK + threadIdx.x of the owned tiles.  false: the whole workgroup lies in a tile beyond the image's
// grid (BLOCK divides TILE_SLOTS, so a workgroup has one tile).  `live`: the slot is inside the image; else (x, yi) is clamped into it
RENE_DEV bool pass_pixel(const TileGrid& G, uint32_t& x, uint32_t& yi, bool& live) {
  static_assert(TILE_SLOTS % BLOCK == 0, "a workgroup's slots lie in one tile");
  const uint32_t w = blockIdx.x * BLOCK + threadIdx.x;
  const uint32_t tile = G.shard_rank + (w >> 10) * G.shard_count, r = w & (TILE_SLOTS - 1u);  // owned tile k is image tile shard_rank + k * shard_count
  const uint32_t tx = tile % G.tiles_x, ty = tile / G.tiles_x;
  if (ty * RENE_TILE_SIZE >= G.height) return false;
  x = slot_x(tx, r), yi = slot_yi(ty, r);
  live = x < G.width && yi < G.height;
  x = min(x, G.width - 1u), yi = min(yi, G.height - 1u);  // keep the wave converged for the coherent item loop
  return true;
}

// the launch of a pass's kernel in the form the scene takes: `small`, the item loop, which needs no LDS, or `bvh` with its traversal stack column
// [stack_depth][lane].  One workgroup per BLOCK owned slots (n_slots is a multiple of TILE_SLOTS)
template <class Launch>
inline hipError_t launch_pixel_pass(const LaunchConfig& cfg, const SceneView& S, const Launch& L, void (*small)(SceneView, Launch),
                                    void (*bvh)(SceneView, Launch), hipStream_t st) {
  const uint32_t blocks = L.grid.n_slots / BLOCK;
  if (blocks == 0 || L.n_frames == 0) return hipSuccess;
  const bool is_small = (cfg.features & FEAT_SMALL) != 0;
  const size_t lds = is_small ? 0 : (size_t)cfg.stack_depth * BLOCK * sizeof(uint32_t);
  hipLaunchKernelGGL(is_small ? small : bvh, dim3(blocks), dim3(BLOCK), lds, st, S, L);
  return hipGetLastError();
}
