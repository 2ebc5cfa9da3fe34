// tail_cut_dump -- what launch_plan.h's small_scene_item_frames answers, and what item_cut makes of the answer, for the cases on its standard input:
// one `F owned_pixels lanes` per line.  One line out per case: the inputs, the policy's item length, then the frames of every level of the cut with
// the policy in front of it and of the untuned cut (item_frames, the decoding of device_code.inc restated on the host).  Host only
// (tests/test_tail_cut.py).
#include "../launch_plan.h"

#include <cstdio>
#include <string>

namespace {
// the frames of level `level`: device_code.inc, item_frames
uint32_t level_frames(const rene::ItemCut& c, uint32_t F, uint32_t level) {
  if (level < c.n_uniform) return c.level_step;
  const uint32_t l = level - c.n_uniform, rest = F - c.n_uniform * c.level_step;
  const uint32_t begin = F - ((rest + (1u << l) - 1u) >> l);
  const uint32_t end = level + 1u >= c.n_levels ? F : F - ((rest + (2u << l) - 1u) >> (l + 1u));
  return end - begin;
}
std::string levels(const rene::ItemCut& c, uint32_t F) {
  std::string s;
  for (uint32_t l = 0; l < c.n_levels; ++l) s += (l ? "," : "") + std::to_string(level_frames(c, F, l));
  return s;
}
}  // namespace

int main() {
  unsigned F;
  unsigned long long px, lanes;
  while (std::scanf("%u %llu %llu", &F, &px, &lanes) == 3) {
    const uint32_t item = rene::small_scene_item_frames(F, px, lanes);
    const rene::ItemCut with = rene::item_cut(F, true, px, item, false, rene::ItemKnobs{}), untuned = rene::item_cut(F, true, px, 0, false, rene::ItemKnobs{});
    std::printf("F=%u owned_pixels=%llu lanes=%llu -> item_frames=%u levels=%s untuned=%s\n", F, px, lanes, item, levels(with, F).c_str(), levels(untuned, F).c_str());
  }
  return 0;
}
