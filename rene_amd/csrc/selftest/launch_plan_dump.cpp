// launch_plan_dump -- prints what launch_plan.h decides for a fixed list of cases, one line per case: the inputs, then the results.
// tests/test_launch_plan.py compares the output with tests/golden/launch_plans.txt.  The images are bit-identical however a job is cut
// (tests/test_gpu_scenes.py), so a changed cut would show as a slower job and nowhere else: this list is what pins the tuned arithmetic.
//   launch_plan_dump <block size of the render kernels>
#include "../launch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <string>

namespace {
using Knob = std::optional<int>;
const Knob none;

std::string show(const Knob& k) { return k ? std::to_string(*k) : std::string("-"); }

void share(uint32_t first_frame, uint32_t n_frames, uint32_t mode, uint32_t rank, uint32_t count) {
  const rene::FrameShare s = rene::frame_share(first_frame, n_frames, mode, rank, count);
  std::printf("share first_frame=%u n_frames=%u mode=%s rank=%u count=%u -> first=%u stride=%u count=%u chain_phase=%u group_frames=%u\n", first_frame, n_frames,
              mode == RENE_SHARD_FRAMES ? "frames" : "tiles", rank, count, s.first, s.stride, s.count, s.chain_phase(), s.group_frames());
}

void cut(uint32_t F, bool small_scene, uint64_t owned_pixels, uint32_t item_frames, bool single_level, Knob item = none, Knob tail = none, Knob levels = none) {
  const rene::ItemCut c = rene::item_cut(F, small_scene, owned_pixels, item_frames, single_level, rene::ItemKnobs{item, tail, levels});
  std::printf("cut F=%u scene=%s owned_pixels=%llu item_frames=%s single_level=%d RENE_ITEM_FRAMES=%s RENE_ITEM_TAIL=%s RENE_LEVELS=%s -> level_step=%u n_uniform=%u n_levels=%u\n", F,
              small_scene ? "small" : "bvh", (unsigned long long)owned_pixels, item_frames == rene::kWholeLaunch ? "whole" : std::to_string(item_frames).c_str(), (int)single_level,
              show(item).c_str(), show(tail).c_str(), show(levels).c_str(), c.level_step, c.n_uniform, c.n_levels);
}

void batch(uint32_t n_levels, uint32_t owned_tiles, uint32_t grid_max, uint32_t block, Knob knob) {
  const uint32_t n_work = owned_tiles * rene::TILE_SLOTS * rene::CHAINS;  // RenderParams::n_work
  const rene::WorkBatch b = rene::work_batch(n_levels, n_work, grid_max, block, knob);
  std::printf("batch n_levels=%u owned_tiles=%u n_work=%u grid_max=%u block=%u RENE_WORK_BATCH=%s -> grid=%u work_batch=%u level_batches=%u\n", n_levels, owned_tiles, n_work, grid_max, block,
              show(knob).c_str(), b.grid, b.work_batch, b.level_batches);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 || std::atoi(argv[1]) < 64) {
    std::fprintf(stderr, "usage: launch_plan_dump <block size of the render kernels>\n");
    return 2;
  }
  const uint32_t block = (uint32_t)std::atoi(argv[1]);

  // ---- the frame share: unsharded and tile shards take the whole range; a frame shard every count-th frame from the first with f % count == rank
  const uint32_t firsts[] = {0u, 5u, 13u}, lengths[] = {1u, 3u, 16u};
  for (uint32_t first : firsts)
    for (uint32_t n : lengths) {
      share(first, n, RENE_SHARD_TILES, 0, 1);
      share(first, n, RENE_SHARD_TILES, 1, 3);
      share(first, n, RENE_SHARD_FRAMES, 0, 1);  // (one frame shard: no shard)
      share(first, n, RENE_SHARD_FRAMES, 0, 2);
      share(first, n, RENE_SHARD_FRAMES, 1, 2);
      share(first, n, RENE_SHARD_FRAMES, 2, 3);
      share(first, n, RENE_SHARD_FRAMES, 5, 8);
    }
  share(6, 16, RENE_SHARD_FRAMES, 0, 3);            // skip = 0
  share(5, 16, RENE_SHARD_FRAMES, 1, 3);            // 0 < skip = 2 < n
  share(5, 2, RENE_SHARD_FRAMES, 0, 4);             // skip = 3 >= n: an empty share
  share(5, 3, RENE_SHARD_FRAMES, 0, 4);             // skip = n
  share(5, 4, RENE_SHARD_FRAMES, 0, 4);             // skip = n - 1: one frame
  share(0xfffffff0u, 15, RENE_SHARD_FRAMES, 3, 8);  // the end of the u32 range
  share(0xffff0000u, 65535, RENE_SHARD_TILES, 0, 1);  // (unsharded: shard_count 1)
  share(65536, 65536, RENE_SHARD_FRAMES, 7, 8);

  // ---- the item cut
  const uint32_t Fs[] = {1u, 2u, 3u, 4u, 5u, 13u, 16u, 63u, 64u, 65u, 128u, 512u, 1024u, 8192u};
  const uint64_t px_small = 256u * 256u, px[] = {(3u << 18) - 1u, 3u << 18, (3u << 19) - 1u, 3u << 19};
  for (uint32_t F : Fs) {  // untuned, no knob
    cut(F, true, px_small, 0, false);
    cut(F, false, px_small, 0, false);
  }
  for (uint32_t F : {13u, 64u, 128u, 512u, 1024u, 8192u})  // the BVH kernels' items shrink with the pixels the context owns
    for (uint64_t p : px) {
      cut(F, false, p, 0, false);
      if (F == 1024u) cut(F, true, p, 0, false);
    }
  for (uint32_t tuned : {16u, 256u, rene::kWholeLaunch})  // rene_tune's choice
    for (uint32_t F : {3u, 5u, 13u, 64u, 65u, 512u, 8192u}) {
      cut(F, true, px_small, tuned, false);
      cut(F, false, px[3], tuned, false);
    }
  for (uint32_t F : {1u, 5u, 64u, 1024u}) {  // RENE_FLAG_SINGLE_LEVEL
    cut(F, true, px_small, 0, true);
    cut(F, false, px[3], 0, true);
    cut(F, true, px_small, 16, true, 4, 1, 5);
  }
  for (int levels : {1, 2, 5, 31, 5000, 0, -3})  // RENE_LEVELS: more levels than frames at F = 13, more than MAX_LEVELS at 5000
    for (uint32_t F : {13u, 1024u, 8192u}) {
      cut(F, true, px_small, 0, false, none, none, levels);
      cut(F, false, px[3], 0, false, none, none, levels);
    }
  cut(13, true, px_small, 64, false, 3, 2, 5);                      // (RENE_LEVELS wins over the other two)
  cut(13, true, px_small, rene::kWholeLaunch, false, 4, 1, none);  // (a whole-launch item wins over the knobs)
  const int pairs[][2] = {{4, 1}, {13, 2}, {5, 5}, {3, 2}, {64, 8}};  // tests/test_gpu_scenes.py's (item, tail) at F = 13
  for (const auto& p : pairs) {
    cut(13, true, px_small, 0, false, p[0], p[1]);
    cut(13, false, px_small, 0, false, p[0], p[1]);
  }
  for (uint32_t F : {1024u, 1025u, 8192u}) {  // K + H > MAX_LEVELS: the loop that lengthens the items
    cut(F, true, px_small, 0, false, 1);
    cut(F, false, px[3], 0, false, 1);
    cut(F, true, px_small, 0, false, 1, 1);
    cut(F, true, px_small, 0, false, 2, 1);
    cut(F, true, px_small, 0, false, 0, 0);  // (knobs below 1 count as 1)
  }
  cut(64, true, px_small, 0, false, 16, 2);    // tail < item, F >= 2 item: the last uniform item joins the rest
  cut(65, true, px_small, 0, false, 16, 4);
  cut(100, true, px_small, 0, false, 16, 1);   // (the halving stops at 16 items)
  cut(8192, true, px_small, 0, false, 4096, 1);
  cut(64, true, px_small, 0, false, 64, 8);    // tail < item, K == 1 && R == 0: a launch of one item's length is halved
  cut(64, false, px[3], 64, false, none, 8);
  cut(100, true, px_small, 0, false, 64, 8);   // tail < item, neither: K = 1, R = 36
  cut(63, true, px_small, 0, false, 64, 8);    // item clipped to F, then K == 1 && R == 0
  cut(64, true, px_small, 0, false, 16, 32);   // tail > item: uniform items and a rest
  cut(70, true, px_small, 0, false, none, 16); // the tail knob alone

  // ---- the batch: 1080p owns 2040 tiles; 2^18 tiles with hundreds of levels need batches above 64 to stay below 2^31 of them
  for (uint32_t tiles : {1u, 3u, 2040u, 1u << 18})
    for (uint32_t levels : {1u, 16u, 300u, 1023u})
      for (uint32_t grid_max : {2048u, 64u})
        for (Knob k : {none, Knob(16), Knob(100), Knob(1024)}) batch(levels, tiles, grid_max, block, k);
  for (int k : {0, 15, 17, 64, 128, 5000}) {  // the knob's clamp and its rounding down to a power of two
    batch(16, 2040, 2048, block, k);
    batch(1, 1, 2048, block, k);
  }
  return 0;
}
