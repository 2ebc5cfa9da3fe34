// exr_zips_check -- host only, no GPU: rene_exr_compress_host over some hundreds of random and crafted bodies, every chunk of every tail inflated
// again with zlib's uncompress and compared with the pre-processed row it came from; the offsets followed, the chunks back to back, `written` exact;
// and exr_deflate.h's closed form of the length code against RFC 1951's table.  It exists to be built with the host code under a sanitizer
// (`make selftest/exr_zips_check_asan` links it with rene_hip.cpp compiled with -fsanitize=address,undefined) and run as a program of its own
// (tests/test_exr_zips_host.py).  Exit status 0 and "ok: ..." on success.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../../include/rene_hip.h"
#include "../exr_deflate.h"

namespace {
int failures = 0;
void expect(bool ok, const char* what, unsigned a = 0, unsigned b = 0) {
  if (ok) return;
  if (++failures <= 20) std::fprintf(stderr, "FAILED: %s (%u, %u)\n", what, a, b);
}
struct Rng {  // xorshift64*
  uint64_t s;
  uint32_t next() {
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
  }
  uint32_t below(uint32_t n) { return next() % n; }
};

uint32_t bytes_per_pixel(uint32_t layers) {
  uint32_t bpp = 0;
  rene_exr_layout(1, 1, layers, nullptr, nullptr, &bpp);
  return bpp;
}

// a row of `kind`: 0 random bytes, 1 one repeating pixel pattern, 2 runs of random lengths, 3 constant, 4 random with a constant stretch
void fill_row(Rng& g, uint8_t* raw, uint32_t n, uint32_t kind) {
  switch (kind) {
    case 0:
      for (uint32_t i = 0; i < n; ++i) raw[i] = (uint8_t)g.next();
      break;
    case 1: {
      uint8_t pat[4] = {(uint8_t)g.next(), (uint8_t)g.next(), (uint8_t)g.next(), (uint8_t)g.next()};
      for (uint32_t i = 0; i < n; ++i) raw[i] = pat[i & 3u];
      break;
    }
    case 2:
      for (uint32_t i = 0; i < n;) {
        const uint32_t run = 1u + g.below(g.below(4) ? 8u : 700u);
        const uint8_t v0 = (uint8_t)g.next(), v1 = (uint8_t)g.next();
        for (uint32_t k = 0; k < run && i < n; ++k, ++i) raw[i] = (i & 1u) ? v1 : v0;
      }
      break;
    case 3:
      std::memset(raw, (int)g.below(256), n);
      break;
    default: {
      for (uint32_t i = 0; i < n; ++i) raw[i] = (uint8_t)g.next();
      const uint32_t a = g.below(n), b = a + g.below(n - a + 1u);
      std::memset(raw + a, 0x3c, b - a);
    }
  }
}

// one body through the library and back; returns the rows stored raw
uint32_t check_body(uint32_t w, uint32_t h, uint32_t layers, const std::vector<uint8_t>& body) {
  size_t header_bytes = 0, body_bytes = 0;
  uint32_t bpp = 0;
  expect(rene_exr_layout(w, h, layers, &header_bytes, &body_bytes, &bpp) == RENE_OK && body_bytes == body.size(), "layout");
  const size_t attr = header_bytes - 8u * (size_t)h, bound = rene_exr_tail_bound(w, h, layers);
  expect(bound == 8u * (size_t)h + body_bytes, "bound");
  const uint32_t n = w * bpp;
  std::vector<uint8_t> tail(bound + 16u, 0xA5);
  size_t written = 0;
  expect(rene_exr_compress_host(w, h, layers, RENE_EXR_COMPRESSION_ZIPS, body.data(), body.size(), tail.data(), bound, &written) == RENE_OK, "compress");
  expect(written >= 8u * (size_t)h && written <= bound, "written within the bound");
  for (size_t i = written; i < tail.size(); ++i)
    if (tail[i] != 0xA5) {
      expect(false, "a byte behind `written` was touched", (unsigned)i);
      break;
    }
  std::vector<uint8_t> d(n), inflated(n + 16u);
  size_t at = 8u * (size_t)h;
  uint32_t stored = 0;
  for (uint32_t y = 0; y < h; ++y) {
    uint64_t off = 0;
    std::memcpy(&off, tail.data() + 8u * (size_t)y, 8);
    expect(off == attr + at, "offset", y);
    if (at + 8u > written) {
      expect(false, "chunk beyond written", y);
      break;
    }
    int32_t prefix[2];
    std::memcpy(prefix, tail.data() + at, 8);
    expect(prefix[0] == (int32_t)y && prefix[1] > 0 && (uint32_t)prefix[1] <= n && at + 8u + (size_t)prefix[1] <= written, "prefix", y);
    if (failures) break;
    const uint8_t* raw = body.data() + (size_t)y * (8u + (size_t)n) + 8u;
    const uint8_t* chunk = tail.data() + at + 8u;
    if ((uint32_t)prefix[1] == n) {
      expect(std::memcmp(chunk, raw, n) == 0, "raw row", y);
      ++stored;
    } else {
      uLongf len = (uLongf)inflated.size();
      const int rc = uncompress(inflated.data(), &len, chunk, (uLong)prefix[1]);
      expect(rc == Z_OK && len == n, "uncompress", y, (unsigned)rc);
      uint8_t prev = 0;
      for (uint32_t i = 0; i < n; ++i) {
        const uint8_t t = raw[rene::zips_raw_index(i, n)];
        d[i] = i ? (uint8_t)(t - prev + 128u) : t;
        prev = t;
      }
      expect(rc == Z_OK && len == n && std::memcmp(inflated.data(), d.data(), n) == 0, "inflated row", y);
    }
    at += 8u + (size_t)prefix[1];
  }
  expect(at == written, "the chunks end at `written`");
  return stored;
}

std::vector<uint8_t> make_body(Rng& g, uint32_t w, uint32_t h, uint32_t layers, int kind) {
  const uint32_t n = w * bytes_per_pixel(layers);
  std::vector<uint8_t> body((size_t)h * (8u + n));
  for (uint32_t y = 0; y < h; ++y) {
    uint8_t* row = body.data() + (size_t)y * (8u + n);
    const uint32_t prefix[2] = {y, n};
    std::memcpy(row, prefix, 8);
    fill_row(g, row + 8, n, kind < 0 ? g.below(5) : (uint32_t)kind);
  }
  return body;
}
}  // namespace

int main() {
  // the closed form of the length code against the table of RFC 1951, section 3.2.5
  static const uint32_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  static const uint32_t extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  for (uint32_t len = 3; len <= 258; ++len) {
    uint32_t k = 28;
    while (base[k] > len) --k;
    uint32_t nb = 0, ns = 0;
    const uint32_t got = rene::zips_match(len, &nb), sym = rene::zips_symbol(257u + k, &ns);
    const uint32_t want = sym | ((len - base[k]) << ns) | (16u << (ns + extra[k]));
    expect(nb == ns + extra[k] + 5u && got == want, "length code", len);
  }
  Rng g{0x9E3779B97F4A7C15ull};
  unsigned bodies = 0, rows = 0, stored = 0;
  static const uint32_t masks[] = {RENE_EXR_ALPHA, RENE_EXR_BEAUTY, RENE_EXR_BEAUTY | RENE_EXR_DEPTH, RENE_EXR_IDS, RENE_EXR_ALL};
  // crafted: every row kind on films 1 x 1 .. , odd widths, rows around the lengths at which the parse changes
  static const uint32_t widths[] = {1, 2, 3, 5, 23, 77, 129, 130, 131, 258, 259, 260, 515, 1031};
  for (uint32_t m : masks)
    for (uint32_t w : widths)
      for (int kind = 0; kind < 5; ++kind) {
        const uint32_t h = 1u + g.below(3);
        stored += check_body(w, h, m, make_body(g, w, h, m, kind));
        ++bodies, rows += h;
      }
  // random films
  for (int k = 0; k < 150; ++k) {
    const uint32_t w = 1u + g.below(g.below(8) ? 200u : 3000u), h = 1u + g.below(6), m = 1u + g.below(255);
    stored += check_body(w, h, m, make_body(g, w, h, m, -1));
    ++bodies, rows += h;
  }
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("ok: %u bodies, %u rows (%u stored raw), every compressed row inflated by zlib to the pre-processed row\n", bodies, rows, stored);
  return 0;
}
