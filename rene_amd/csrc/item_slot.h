// item_slot.h -- the arithmetic between a work id, a pixel slot and a pixel, as plain functions the device code (device_code.inc, the work-item
// switch of render_kernel) and a host program (selftest/item_slot_check.cpp) compile alike.  A level's work id is slot * CHAINS + chain; a slot is
// k << 10 | r: owned tile k (image tile shard_rank + k * shard_count), place r inside it (device_scene.h, pixel slots).
#pragma once
#include <stdint.h>

#include "../../include/rene_hip.h"
#include "device_scene.h"

#if defined(__HIPCC__)
#define RENE_HD __host__ __device__ __forceinline__
#else
#define RENE_HD inline
#endif

namespace rene {

// x / n for x < 2^31 and a quotient below 2^22, through the reciprocal the host supplies (inv = 1.0f / n): the float
// estimate is off by at most one, the remainder says which way.  Replaces the ~24-instruction expansion of an
// integer division in the work-item bookkeeping.
RENE_HD uint32_t udiv_small(uint32_t x, uint32_t n, float inv, uint32_t& rem) {
  uint32_t q = (uint32_t)((float)x * inv);
  int32_t r = (int32_t)(x - q * n);
  if (r < 0) { q--; r += (int32_t)n; }
  if (r >= (int32_t)n) { q++; r -= (int32_t)n; }
  rem = (uint32_t)r;
  return q;
}

// place r (0 .. 1023) of image tile (tx, ty) -> the pixel: 8x8 micro-tiles, four to a row -- the inverse of tile_slot()
RENE_HD uint32_t slot_x(uint32_t tx, uint32_t r) {
  const uint32_t sub = r >> 6, l = r & 63u;
  return tx * RENE_TILE_SIZE + (sub & 3u) * 8u + (l & 7u);
}
RENE_HD uint32_t slot_yi(uint32_t ty, uint32_t r) {  // the image row, top first
  const uint32_t sub = r >> 6, l = r & 63u;
  return ty * RENE_TILE_SIZE + (sub >> 2) * 8u + (l >> 3);
}

// The slot of pixel (x, yi) -- yi the image row, top first -- of a tile the context owns: its owned-tile index (t - shard_rank) / shard_count is exact,
// so a float reciprocal rounded to the nearest integer finds it (t < 2^18)
RENE_HD uint32_t owned_tile_index(uint32_t t, uint32_t shard_rank, float inv_shard_count) { return (uint32_t)((float)(t - shard_rank) * inv_shard_count + 0.5f); }
RENE_HD uint32_t pixel_slot_of(uint32_t x, uint32_t yi, uint32_t tiles_x, uint32_t shard_rank, float inv_shard_count) {
  const uint32_t t = (yi >> 5) * tiles_x + (x >> 5);
  return (owned_tile_index(t, shard_rank, inv_shard_count) << 10) | tile_slot(x, yi);
}

}  // namespace rene
