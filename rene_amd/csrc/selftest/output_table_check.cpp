// output_table_check -- host only: the argument the device's sRGB transform rests on (kernels_output.hip), checked on EVERY non-negative finite float.
//   1. rene_output_thresholds' table has 255 strictly increasing positive floats, the last at most 1;
//   2. for every float v from +0 to FLT_MAX, in order: the number of thresholds T[k] <= v equals rene_to_rgb8(v) with n_samples 1;
//   3. rene_to_rgb8 over those floats never goes down and goes up exactly 255 times, by one each time.
// The range of bit patterns 0 .. 0x7f7fffff is cut into one contiguous piece per thread (at most 16); a piece is evaluated in blocks through the
// library's own rene_to_rgb8.  Exit status 0 and one line "ok ..." on success; the first mismatch and status 1 otherwise.
// (tests/test_output_host.py runs it.)
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../../include/rene_hip.h"

namespace {

constexpr uint64_t kEnd = 0x7f800000ull;  // one past the bits of FLT_MAX
constexpr size_t kBlock = 1u << 16;

struct Piece {
  uint64_t steps = 0;      // places inside the piece where the byte goes up
  uint8_t first = 0, last = 0;
  bool ok = true;
  char what[160] = {0};
};

float of_bits(uint32_t b) {
  float v;
  std::memcpy(&v, &b, sizeof v);
  return v;
}

void run(const float* T, uint64_t lo, uint64_t hi, Piece* out, std::atomic<bool>* stop) {
  std::vector<float> v(kBlock);
  std::vector<uint8_t> b(kBlock);
  uint32_t count = (uint32_t)(std::upper_bound(T, T + 255, of_bits((uint32_t)lo)) - T);  // thresholds <= the piece's first float
  bool have_prev = false;
  uint8_t prev = 0;
  for (uint64_t at = lo; at < hi && !stop->load(std::memory_order_relaxed); at += kBlock) {
    const size_t n = (size_t)std::min<uint64_t>(kBlock, hi - at);
    for (size_t i = 0; i < n; ++i) v[i] = of_bits((uint32_t)(at + i));
    rene_to_rgb8(v.data(), n, 1u, b.data());
    for (size_t i = 0; i < n; ++i) {
      while (count < 255u && v[i] >= T[count]) ++count;  // (the floats come in order: the count only grows)
      if (b[i] != count) {
        std::snprintf(out->what, sizeof out->what, "bits 0x%08x (%.9g): rene_to_rgb8 gives %u, the table %u", (unsigned)(at + i), (double)v[i], (unsigned)b[i], count);
        out->ok = false;
        stop->store(true);
        return;
      }
      if (have_prev && b[i] != prev) {
        if (b[i] != prev + 1) {
          std::snprintf(out->what, sizeof out->what, "bits 0x%08x (%.9g): rene_to_rgb8 goes from %u to %u", (unsigned)(at + i), (double)v[i], (unsigned)prev, (unsigned)b[i]);
          out->ok = false;
          stop->store(true);
          return;
        }
        ++out->steps;
      }
      if (!have_prev) out->first = b[i];
      have_prev = true;
      prev = b[i];
    }
  }
  out->last = prev;
}

}  // namespace

int main() {
  float T[255];
  rene_output_thresholds(T);
  for (int k = 0; k < 255; ++k)
    if (!(T[k] > 0.0f) || (k && !(T[k] > T[k - 1])) || !(T[k] <= 1.0f)) {
      std::printf("threshold %d = %.9g is out of order or out of (0, 1]\n", k, (double)T[k]);
      return 1;
    }
  const unsigned n_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<Piece> pieces(n_threads);
  std::vector<std::thread> threads;
  std::atomic<bool> stop{false};
  // most of the work is below 1.0f, where the host takes its pow on a fraction: the pieces are cut evenly over the patterns all the same
  for (unsigned t = 0; t < n_threads; ++t) threads.emplace_back(run, T, kEnd * t / n_threads, kEnd * (t + 1) / n_threads, &pieces[t], &stop);
  for (std::thread& th : threads) th.join();
  uint64_t steps = 0;
  for (unsigned t = 0; t < n_threads; ++t) {
    if (!pieces[t].ok) {
      std::printf("%s\n", pieces[t].what);
      return 1;
    }
    steps += pieces[t].steps;
    if (t) {
      const int d = (int)pieces[t].first - (int)pieces[t - 1].last;
      if (d < 0 || d > 1) {
        std::printf("rene_to_rgb8 goes from %u to %u between two pieces\n", (unsigned)pieces[t - 1].last, (unsigned)pieces[t].first);
        return 1;
      }
      steps += (uint64_t)d;
    }
  }
  if (pieces[0].first != 0 || pieces[n_threads - 1].last != 255 || steps != 255) {
    std::printf("rene_to_rgb8 runs from %u to %u in %llu steps, not from 0 to 255 in 255\n", (unsigned)pieces[0].first, (unsigned)pieces[n_threads - 1].last, (unsigned long long)steps);
    return 1;
  }
  std::printf("ok: %llu floats, 255 steps, %u threads\n", (unsigned long long)kEnd, n_threads);
  return 0;
}
