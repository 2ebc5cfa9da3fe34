// item_slot_check -- what the work-item switch of the Matte small-scene kernels rests on (device_code.inc, item_switch; item_slot.h), on the host:
// for films from 1x1 to 16384x16384, ragged ones included, tile shard counts 1, 2, 3, 5 and 8 and every rank, and EVERY slot of every owned tile
//   - the slot a lane keeps is the slot pixel_slot() rebuilds: pixel_slot_of(decode(slot)) == slot, with the owned-tile index rounded as the host's
//     compiler rounds it (multiply, then add) and as the device's does (one fused multiply-add);
//   - the tile division of the take (udiv_small, through the host's reciprocal) gives the integer quotient and remainder.
// The largest film has 2^18 tiles, the bound the float reciprocals are documented for.  Prints one line per film and the number of mismatches;
// exit status 1 if there are any (tests/test_item_slot.py).
#include "../item_slot.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>

namespace {
using namespace rene;

uint32_t owned_tiles(uint32_t n_tiles, uint32_t rank, uint32_t count) { return n_tiles > rank ? (n_tiles - rank + count - 1u) / count : 0u; }

struct Film {
  uint32_t w, h;
};

// the mismatches of owned tiles [k0, k1) of one (film, shard)
uint64_t check_tiles(Film f, uint32_t rank, uint32_t count, uint32_t k0, uint32_t k1) {
  const uint32_t tiles_x = (f.w + RENE_TILE_SIZE - 1) / RENE_TILE_SIZE;
  const float inv_tiles_x = 1.0f / (float)std::max(1u, tiles_x), inv_shard_count = 1.0f / (float)count;  // (rene_hip.cpp, the launch's RenderParams)
  uint64_t bad = 0;
  for (uint32_t k = k0; k < k1; ++k) {
    const uint32_t tile = rank + k * count;
    uint32_t tx = 0;
    const uint32_t ty = udiv_small(tile, tiles_x, inv_tiles_x, tx);
    bad += ty != tile / tiles_x || tx != tile % tiles_x;
    for (uint32_t r = 0; r < TILE_SLOTS; ++r) {
      const uint32_t slot = (k << 10) | r;
      const uint32_t x = slot_x(tx, r), yi = slot_yi(ty, r);
      // (a slot of a ragged tile outside the film is never rendered: the identity holds for it all the same)
      const uint32_t t = (yi >> 5) * tiles_x + (x >> 5);
      const uint32_t k_fused = (uint32_t)std::fma((float)(t - rank), inv_shard_count, 0.5f);
      bad += pixel_slot_of(x, yi, tiles_x, rank, inv_shard_count) != slot;
      bad += ((k_fused << 10) | tile_slot(x, yi)) != slot;
      bad += t != tile || x - tx * RENE_TILE_SIZE >= RENE_TILE_SIZE || yi - ty * RENE_TILE_SIZE >= RENE_TILE_SIZE;
    }
  }
  return bad;
}

uint64_t check_film(Film f, unsigned n_threads) {
  const uint32_t tiles_x = (f.w + RENE_TILE_SIZE - 1) / RENE_TILE_SIZE, tiles_y = (f.h + RENE_TILE_SIZE - 1) / RENE_TILE_SIZE, n_tiles = tiles_x * tiles_y;
  std::atomic<uint64_t> bad{0}, slots{0};
  for (uint32_t count : {1u, 2u, 3u, 5u, 8u})
    for (uint32_t rank = 0; rank < count; ++rank) {
      const uint32_t owned = owned_tiles(n_tiles, rank, count);
      const uint32_t per = (owned + n_threads - 1) / n_threads;
      std::vector<std::thread> pool;
      for (uint32_t k0 = 0; k0 < owned; k0 += std::max(1u, per))
        pool.emplace_back([&, k0] { bad += check_tiles(f, rank, count, k0, std::min(owned, k0 + std::max(1u, per))); });
      for (std::thread& t : pool) t.join();
      slots += (uint64_t)owned * TILE_SLOTS;
    }
  std::printf("film %ux%u tiles=%u slots_checked=%llu mismatches=%llu\n", f.w, f.h, n_tiles, (unsigned long long)slots.load(), (unsigned long long)bad.load());
  return bad;
}

}  // namespace

int main() {
  const unsigned n_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  uint64_t bad = 0;
  for (Film f : {Film{1, 1}, Film{31, 33}, Film{32, 32}, Film{100, 70}, Film{33, 4097}, Film{1024, 1024}, Film{16384, 1}, Film{1, 16384}, Film{4001, 4097}, Film{16384, 16384}})
    bad += check_film(f, n_threads);
  std::printf("mismatches %llu\n", (unsigned long long)bad);
  return bad ? 1 : 0;
}
