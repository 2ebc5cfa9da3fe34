// exr_deflate.h -- what the host's rene_exr_compress_host (rene_hip.cpp) and the device's ZIPS kernels (kernels_exr_zips.hip) share: OpenEXR's ZIP
// pre-processing as an index map, the fixed Huffman code of RFC 1951 and the closed form that turns a position of the pre-processed row into its
// token.  The stream is specified in include/rene_hip.h (compressed OpenEXR output); nothing here keeps state from one position to the next.
//
//   raw   the row's n bytes (n even) as the uncompressed body holds them
//   t     raw[0::2] ++ raw[1::2];  t[i] = raw[zips_raw_index(i, n)]
//   d     d[0] = t[0], d[i] = (t[i] - t[i-1] + 128) mod 256
//   e     e[i] = i >= 2 and d[i] == d[i-2]
// A position i with e[i] == 0 is a literal.  Inside a maximal interval of e == 1 that starts at s, with r = (i - s) mod 258 and f the distance from i
// to the interval's end (the first position behind it; f >= 1), the 258-byte piece i lies in holds min(r + f, 258) positions of the interval:
//   r == 0, f >= 3   a match of length min(f, 258), distance 2
//   r == 0, f <  3   a literal
//   r == 1, f == 1   a literal (the second of a two-byte rest)
//   otherwise        nothing: the position is inside a match
// f is only ever compared with 1, 2 and 258, so a look-ahead of 258 positions decides every token.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RENE_ZIPS_HD __host__ __device__ __forceinline__
#else
#define RENE_ZIPS_HD inline
#endif

namespace rene {

constexpr uint32_t ZIPS_MAX_MATCH = 258, ZIPS_MIN_MATCH = 3;
constexpr uint32_t ZIPS_ADLER_MOD = 65521;
// the 19 bits in front of the first token, LSB first: the zlib header 0x78 0x01, then BFINAL = 1 and BTYPE = 01 (the bits 1, 1, 0)
constexpr uint32_t ZIPS_HEAD_BITS = 19, ZIPS_HEAD = 0x0178u | (0x3u << 16);
constexpr uint32_t ZIPS_EOB_BITS = 7;  // symbol 256: seven zero bits

// where t[i] lies in raw
RENE_ZIPS_HD uint32_t zips_raw_index(uint32_t i, uint32_t n) {
  const uint32_t h = n >> 1;
  return i < h ? 2u * i : 2u * (i - h) + 1u;
}

// the n low bits of v in reverse order (n <= 16): a Huffman code, which goes MSB first, as the value an LSB-first writer appends
RENE_ZIPS_HD uint32_t zips_reverse(uint32_t v, uint32_t n) {
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
  v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
  return v >> (16u - n);
}

// the fixed code of literal / length symbol `sym` (0 .. 287), as written; *bits = its length
RENE_ZIPS_HD uint32_t zips_symbol(uint32_t sym, uint32_t* bits) {
  uint32_t code, n;
  if (sym < 144u) code = 0x30u + sym, n = 8u;
  else if (sym < 256u) code = 0x190u + (sym - 144u), n = 9u;
  else if (sym < 280u) code = sym - 256u, n = 7u;
  else code = 0xC0u + (sym - 280u), n = 8u;
  *bits = n;
  return zips_reverse(code, n);
}

// a match of `len` (3 .. 258) at distance 2, as written: the length symbol, its extra bits, then distance code 1 (five bits, no extra bits)
RENE_ZIPS_HD uint32_t zips_match(uint32_t len, uint32_t* bits) {
  uint32_t sym, extra = 0u, extra_bits = 0u;
  if (len <= 10u) sym = 254u + len;
  else if (len == ZIPS_MAX_MATCH) sym = 285u;
  else {  // 265 .. 284 in groups of four, one more extra bit per group: base = 3 + ((4 + k) << eb)
    const uint32_t l = len - 3u;  // 8 .. 254
    uint32_t eb = 1u;
    while ((l >> (eb + 3u)) != 0u) ++eb;  // floor(log2 l) - 2
    sym = 261u + 4u * eb + ((l >> eb) & 3u);
    extra = l & ((1u << eb) - 1u), extra_bits = eb;
  }
  uint32_t n;
  uint32_t v = zips_symbol(sym, &n);
  v |= extra << n, n += extra_bits;
  v |= 16u << n, n += 5u;  // 00001 MSB first
  *bits = n;
  return v;
}

// the token of a position: its bits as written and their number (0: the position is inside a match).  d: its byte; e: see above; r, f: for e != 0
RENE_ZIPS_HD uint32_t zips_token(uint32_t d, bool e, uint32_t r, uint32_t f, uint32_t* bits) {
  if (e) {
    if (r == 0u && f >= ZIPS_MIN_MATCH) return zips_match(f < ZIPS_MAX_MATCH ? f : ZIPS_MAX_MATCH, bits);
    if (!((r == 0u) || (r == 1u && f == 1u))) {
      *bits = 0u;
      return 0u;
    }
  }
  return zips_symbol(d, bits);
}

// the zlib stream's length for `token_bits` bits of tokens
RENE_ZIPS_HD uint64_t zips_stream_bytes(uint64_t token_bits) { return (ZIPS_HEAD_BITS + token_bits + ZIPS_EOB_BITS + 7u) / 8u + 4u; }

}  // namespace rene
