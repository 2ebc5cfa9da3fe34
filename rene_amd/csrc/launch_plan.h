// launch_plan.h -- the arithmetic of a render launch, on its own: which frames of a request are a context's, how a chain's frames are cut into work
// items, and in what batches the work ids are handed out.  Host only and pure: no HIP, no environment, no context -- rene_render reads the knobs and
// the context and passes them in, and assigns RenderParams from these results.  The images do not depend on any of it (they are bit-identical however
// a job is cut, tests/test_gpu_scenes.py); its speed does -- the comments carry the measurements -- and tests/test_launch_plan.py pins every branch
// (selftest/launch_plan_dump.cpp against tests/golden/launch_plans.txt).
#pragma once
#include <algorithm>
#include <optional>

#include "../../include/rene_hip.h"
#include "device_scene.h"

namespace rene {

// frames per work item (rene_ctx::item_frames): one item per pixel, chain and launch
constexpr uint32_t kWholeLaunch = 0xffffffffu;

// which frames of [first_frame, first_frame + n_frames) are this context's: all of them, or under RENE_SHARD_FRAMES those
// with f % shard_count == shard_rank.  The kernels compute the frames' seeds themselves (device_math.h, frame_seed).
struct FrameShare {
  uint32_t first, stride, count;
  // frame chains (device_scene.h): global frame f belongs to chain (f / frame_stride) % CHAINS -- a rule on the frame's number, so that a pixel's
  // chains hold the same sums however a job is cut into calls
  uint32_t chain_phase() const { return (first / stride) & (CHAINS - 1u); }
  uint32_t group_frames() const { return (count + CHAINS - 1u) / CHAINS; }  // (what the items cut: the frames of one chain)
};
inline FrameShare frame_share(uint32_t first_frame, uint32_t n_frames, uint32_t shard_mode, uint32_t shard_rank, uint32_t shard_count) {
  if (shard_mode != RENE_SHARD_FRAMES || shard_count <= 1) return FrameShare{first_frame, 1u, n_frames};
  const uint32_t n = shard_count, r = shard_rank;
  const uint32_t skip = (r + n - first_frame % n) % n;  // frames before the first one with f % n == r
  return FrameShare{first_frame + skip, n, skip < n_frames ? (n_frames - skip + n - 1) / n : 0};
}

// every pixel's frames in work items (device_code.inc, item_frames): uniform items of `item` frames, the last one or two of
// them cut into halving items down to `tail` frames; RENE_LEVELS=<n> (tests, A/B measurements) cuts into n uniform items
struct ItemKnobs {
  std::optional<int> item_frames, item_tail, levels;  // RENE_ITEM_FRAMES, RENE_ITEM_TAIL, RENE_LEVELS
};
struct ItemCut {
  uint32_t level_step, n_uniform, n_levels;  // n_uniform items of level_step frames, then n_levels - n_uniform halving items over the rest
};
// F = FrameShare::group_frames() >= 1; item_frames: the context's tuned item length, 0 = not tuned, kWholeLaunch
inline ItemCut item_cut(uint32_t F, bool small_scene, uint64_t owned_pixels, uint32_t item_frames, bool single_level, const ItemKnobs& knobs) {
  // untuned: sixteen items per pixel and launch for the item-loop kernels, 32 for the BVH kernels, at least 16 frames each
  // (measured, one launch per job, MI355X: Cornell 1024 frames flat from 64 to 96 frames per item, veach-mis 4096 frames best at
  // 256 - 341, dragon-class 1024 at 32, the teapot scene 8192 at 256: it is the number of item switches per pixel that a launch
  // pays for, and the length of its last item -- and a BVH scene's pixels differ more in cost);
  // (what "flat from 64 to 96" and the later "96 ahead of 64 by 0.5 ms" meant, profiles/tail_cut_ab.txt: at F = 128 both are TWO items, 64 + 64
  // against 96 + 32 -- the same switches, a last item half as long.  A level beyond two costs about 0.9 ms of that job, a frame of the last item
  // 0.018 - 0.024 ms down to 16 frames, and below that the job grows again by 0.2 ms per halving.  This default stays as it is: the long first and
  // short last item come from small_scene_item_frames below, in front of this function, where they were measured to pay.)
  // no halving tail by default (tail = item): it buys nothing once the hand-off waits are rare (docs/history.md section 4f) -- the halving tails that
  // lost did so through their extra levels, not through the short last item
  // (short launches -- one rank's share of a multi-GPU job -- want few, long items: Cornell 128 frames, 8 / 16 / 32 / 64 frames per
  // item: 6.89 / 6.59 / 6.59 / 6.41 ms; 256 frames, 16 / 32 / 64 / 128: 13.30 / 13.13 / 13.21 / 12.84; 512 frames, 32 / 64 / 128: 24.93 / 24.74 / 25.23)
  // (frame groups: a chain has half the frames and wants items as long as the undivided job's, or longer -- dragon-class, two chains of 512
  // frames: items of 16 / 32 / 64 frames 671 / 653 / 642 ms; the teapot scene, two chains of 4096: 128 / 256 / 512 / 1024 frames 3139 / 3106 / 3179 / 3157 ms)
  // (frame chains, round 4: F is what ONE of a pixel's CHAINS chains renders in this launch; the same item LENGTHS as before -- sixteen / 32 items
  // per pixel and launch over all its chains)
  // (BVH kernels, re-swept with chains on dragon-class, a chain's share F = 128 frames: the whole 2 M-pixel image wants items of 64 frames -- 648 ms
  // against 654 at 32 and 667 at 16 -- and an eighth of its tiles items of 16 -- 93.3 ms against 98.8 at 32 and 108 at 64: what matters is how
  // many items the context's lanes share, so the item shrinks with the pixels the context owns, F / 2 at 2 M pixels down to F / 8)
  const uint32_t bvh_div = owned_pixels >= (3u << 19) ? 2u : owned_pixels >= (3u << 18) ? 4u : 8u;
  uint32_t item = item_frames ? item_frames : (small_scene ? std::max(64u, F / (16u / CHAINS)) : std::max(16u, F / bvh_div));
  uint32_t tail = item;
  // (... and for the BVH kernels a halving tail: with chains the end of the job is the end of its last items, not the heaviest pixel's chain --
  // dragon-class, two chains: items of 64 frames 651 ms, halving down to 8 frames 641; the teapot scene 256 -> 16 frames: 3140 -> 3092 ms)
  if (!small_scene && !item_frames) tail = std::max(4u, item / 8u);
  if (knobs.item_frames) item = (uint32_t)std::max(1, *knobs.item_frames);  // tuning knobs
  if (knobs.item_tail) tail = (uint32_t)std::max(1, *knobs.item_tail);
  if (knobs.levels) {
    const uint32_t levels = std::min((uint32_t)std::max(1, std::min((int)MAX_LEVELS, *knobs.levels)), F);
    item = (F + levels - 1) / levels;
    tail = item;
  }
  if (item_frames == kWholeLaunch || single_level || F < 4) item = tail = F;
  // a version counts at most MAX_LEVELS items (the work ids are decoded per level: no bound from their width, device_code.inc batch_decode)
  const uint32_t max_levels = MAX_LEVELS;
  item = std::min(std::max(item, 1u), F);
  for (;;) {
    uint32_t K = F / item, R = F - K * item, H = R ? 1u : 0u;  // K uniform items, then H halving items over the rest R
    if (tail < item && F >= 2 * item) {  // the last uniform item joins the rest: R in [item, 2 item)
      K -= 1;
      R += item;
      H = 1;
      while (H < 16u && (R >> H) >= tail) ++H;  // the last one has ceil(R / 2^(H-1)) >= tail frames
    } else if (tail < item && K == 1 && R == 0) {  // a launch of one item's length: halve that
      K = 0;
      R = F;
      H = 1;
      while (H < 16u && (R >> H) >= tail) ++H;
    }
    if (K + H <= max_levels) return ItemCut{item, K, K + H};
    item += (item + 7) / 8;  // too many levels: longer items
  }
}

// The policy in front of item_cut for the item-loop kernels of the path integrator (rene_render passes its answer as item_frames when the context is
// not tuned, no knob is set and RENE_FLAG_SINGLE_LEVEL is off): the length of a chain's FIRST item, or 0 = the untuned cut above.
// What it rests on (profiles/tail_cut_ab.txt): with the same number of levels a job is the shorter the shorter its LAST item is -- the end of a
// launch is the stagger of the lanes' last items, 0.02 ms per frame of them on Cornell -- down to where the last level's sweep of the image no
// longer covers the first level's long items: there lanes wait at the hand-off and the job grows again, steeply (the waiting share of the lanes
// says where).  The untuned cut of an even F is two items of F / 2; the policy's is one item of F - last frames and one of `last`: two levels
// for every F, never more than the untuned cut has, and the last item shorter than the first.
// `last`, measured on MI355X with whole jobs of one launch (ms per job; * = the untuned cut), the whole 1024 x 1024 image, 16 items of a level per lane:
//     Cornell   F = 128, last 64* / 32 / 16 / 8 / 4:     36.56 / 35.98 / 35.60 / 35.80 / 35.99      F / 8 best
//     Cornell   F = 256, last 128* / 64 / 32 / 16 / 8:   70.83 / 69.93 / 69.16 / 69.68 / 70.33      F / 8 best
//     veach-mis F = 128, last 64* / 32 / 16 / 8 / 4:     102.90 / 101.57 / 100.60 / 100.10 / 101.21 F / 16 best, F / 8 has 0.8 of its gain
//     veach-mis F = 512, last 256* / 128 / 64 / 32 / 16: 400.86 / 396.95 / 394.27 / 393.48 / 398.00 F / 16 best, F / 8 has 0.9 of its gain; F / 32 falls
//                                                                                                   behind F / 4: the cliff is close to the optimum
// So: F / 8 -- the side of the optimum away from the cliff -- where a level has sixteen items or more per lane, and 0, the untuned cut, wherever
// nothing was measured or nothing was gained: other F, images beyond 2^20 pixels (the BVH scenes' sizes), and fewer items per lane -- one rank's
// eighth of the image's tiles (2 per lane, the share of the bench job on eight GPUs) has 5.35 / 5.35 / 5.49 / 5.63 / 5.78 ms at F = 128: nothing
// to gain at F / 4, and from F / 8 on 2 - 14 % of the lanes wait at the hand-off.
// lanes: the persistent launch's upper bound, workgroups x their size (what the device holds is the same for every launch of a context).
constexpr uint32_t kTailCutMinF = 128, kTailCutMaxF = 512;  // a chain's share of the launch
constexpr uint64_t kTailCutMaxPixels = 1ull << 20;          // owned pixels
constexpr uint64_t kTailCutItemsPerLane = 16;               // items of one level per lane, at least
inline uint32_t small_scene_item_frames(uint32_t F, uint64_t owned_pixels, uint64_t lanes) {
  if (F < kTailCutMinF || F > kTailCutMaxF || lanes == 0) return 0;
  if (owned_pixels > kTailCutMaxPixels || owned_pixels * CHAINS < lanes * kTailCutItemsPerLane) return 0;
  return F - F / 8u;
}

// launch no more lanes than there are work items; hand items out in batches small enough that every
// launched wave gets some (a tile shard of a small image has fewer items than the chip has lanes)
struct WorkBatch {
  uint32_t grid, work_batch, level_batches;
};
// n_work: the work ids of one level (RenderParams::n_work); grid_max: the persistent launch's upper bound in blocks of block_size lanes; knob: RENE_WORK_BATCH
inline WorkBatch work_batch(uint32_t n_levels, uint32_t n_work, uint32_t grid_max, uint32_t block_size, const std::optional<int>& knob) {
  const uint64_t total_items = (uint64_t)n_levels * n_work;  // (up to MAX_LEVELS x 2^31)
  const uint64_t blocks_needed = (total_items + block_size - 1) / block_size;
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(grid_max, blocks_needed));
  const uint32_t waves = grid * (block_size / 64);
  // 64 ids = one wave's worth: every id a wave takes is rendered at once.  (With 128 the second half of a batch sat reserved
  // until lanes of that wave came free, its pixels started late, and the items that continue from them -- handed out one sweep
  // of the image later -- found them unfinished: Cornell 52.1 -> 48.5 ms per job, docs/history.md section 4f.)
  uint32_t batch = 64;
  if (knob) {  // tuning knob (a power of two: it must divide n_work)
    const uint32_t want = (uint32_t)std::max(16, std::min(1024, *knob));
    while (batch * 2u <= want) batch *= 2u;
    while (batch > want) batch >>= 1;
  }
  while (batch > 16 && (uint64_t)batch * waves * 2u > total_items) batch >>= 1;
  while (batch < 1024u && (total_items / batch) >> 31) batch <<= 1;  // fewer than 2^31 batches (only images beyond 2^23 slots with hundreds of levels)
  return WorkBatch{grid, batch, n_work / batch};  // n_work = owned tiles x 1024 x CHAINS: a batch never straddles two levels
}

}  // namespace rene
