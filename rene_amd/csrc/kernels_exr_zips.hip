// kernels_exr_zips.hip -- the ZIPS chunks of a compressed OpenEXR file on the device (rene_exr_compress, include/rene_hip.h): an uncompressed body in,
// the file's tail -- the offset table and the chunks back to back -- out, bit for bit the bytes of the host's rene_exr_compress_host.  The stream
// is specified in the header; exr_deflate.h holds what both sides share.
//
//   Three launches, none of which waits on another workgroup:
//     zips_size_kernel    one workgroup per row: the row's token bits, summed; the chunk's size with the raw fallback decided (sizes[y])
//     zips_scan_kernel    one workgroup: the exclusive sum of the chunks' lengths -- the offset table and `written`
//     zips_encode_kernel  one workgroup per row: the chunk at its final offset -- the bit stream, or the raw row where the size kernel chose that
//   The size and the encode kernel walk a row by the same code (zips_row), so the bytes the second writes are the bytes the first counted.
//
//   A row is streamed in segments of EXR_ZIPS_SEGMENT positions of d, the pre-processed row, which is never stored: a segment's bytes of d are
//   computed from byte loads of raw into LDS, with the two positions before the segment (for e) and the 258 behind it (the look-ahead that decides a
//   match's length).  A thread owns a strip of 16 consecutive positions.  What crosses strips is three block scans: the last position with e == 0
//   at or before the strip (a maximum), the first one behind it (a minimum) and, in the encode kernel, the bits in front of it (a sum); what crosses
//   segments is the last e == 0 position, the partial dword of the bit stream and the two Adler sums -- every loop's bound follows from the row's
//   length.  Adler-32 over a 1 MB row: the sum of (n - i) d[i] reaches 2.6e14, so the partial sums are 64-bit and reduced mod 65521 once.
//
//   The bits of a segment are merged in LDS with ds_or_b32 (a thread's strip starts at any bit; its neighbours' strips share its first and last dword)
//   and leave as aligned dword stores.  A chunk starts at any byte: the bytes of its first and its last dword that are its own leave as single byte
//   stores through a volatile access -- the neighbouring chunks' workgroups write the other bytes of those dwords, and the backend must not join
//   byte stores into a dword store that is not aligned (store_word in kernels_exr.hip has the same trap).  Nothing behind the last chunk is written.
//   Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include "exr_deflate.h"
#include "kernels.h"

namespace rene {

constexpr uint32_t EXR_ZIPS_BLOCK = 256;
constexpr uint32_t EXR_ZIPS_STRIP = 16;      // positions per thread and segment
constexpr uint32_t EXR_ZIPS_SEGMENT = 4096;  // positions of d per segment: EXR_ZIPS_BLOCK x EXR_ZIPS_STRIP
constexpr uint32_t EXR_ZIPS_WAVES = EXR_ZIPS_BLOCK / 64u;
// a segment's bytes of d in LDS: position p of the row at byte p - a + 4 for the segment's first position a (the strips start on dwords)
constexpr uint32_t ZIPS_D_DWORDS = (4u + EXR_ZIPS_SEGMENT + ZIPS_MAX_MATCH + 3u) / 4u;
// the bit buffer: a segment's 9 bits per position at most, the dword carried over, the chunk's start (3 bytes of alignment, the 8-byte prefix, 19
// bits) or its end (7 + 7 + 32 bits)
constexpr uint32_t ZIPS_OUT_DWORDS = (EXR_ZIPS_SEGMENT * 9u + 32u + 24u + 64u + ZIPS_HEAD_BITS + 46u + 31u) / 32u + 1u;
constexpr uint32_t ZIPS_NONE = 0x7fffffffu;  // no e == 0 position

static_assert(EXR_ZIPS_SEGMENT == EXR_ZIPS_BLOCK * EXR_ZIPS_STRIP && EXR_ZIPS_STRIP == 16u, "a strip is four dwords of d");

namespace {

using GlobalByte = volatile __attribute__((address_space(1))) uint8_t;  // (global memory: a volatile generic access would be a flat store)
__device__ __forceinline__ void store_byte(uint8_t* p, uint32_t v) { *(GlobalByte*)reinterpret_cast<uintptr_t>(p) = (uint8_t)v; }

// dword w of a chunk's destination, whose bytes lo .. hi - 1 are the chunk's own
__device__ __forceinline__ void store_chunk_dword(uint8_t* aligned, uint32_t w, uint32_t v, uint32_t lo, uint32_t hi) {
  uint8_t* p = aligned + 4u * (size_t)w;
  if (lo == 0u && hi == 4u) {
    *reinterpret_cast<uint32_t*>(p) = v;
  } else {
    for (uint32_t b = lo; b < hi; ++b) store_byte(p + b, v >> (8u * b));
  }
}

struct ZipsShared {
  uint32_t d[ZIPS_D_DWORDS];
  uint32_t out[ZIPS_OUT_DWORDS];
  int32_t wave_last[EXR_ZIPS_WAVES];
  uint32_t wave_next[EXR_ZIPS_WAVES];
  uint32_t wave_bits[EXR_ZIPS_WAVES];
  uint32_t halo_zero;
  unsigned long long sums[3][EXR_ZIPS_WAVES];
};

__device__ __forceinline__ uint32_t d_byte(const ZipsShared& S, int32_t rel) {  // d at position a + rel of the segment that starts at a (rel >= -4)
  const uint32_t at = (uint32_t)(rel + 4);
  return (S.d[at >> 2] >> (8u * (at & 3u))) & 255u;
}

// One row.  ENCODE: writes the chunk at `chunk` (int32 y, int32 size, the zlib stream) and returns nothing of use; else returns the row's token bits.
template <bool ENCODE>
__device__ __forceinline__ unsigned long long zips_row(ZipsShared& S, const uint8_t* raw, const uint32_t n, const uint32_t y, const uint32_t size, uint8_t* chunk) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n_segments = (n + EXR_ZIPS_SEGMENT - 1u) / EXR_ZIPS_SEGMENT;
  int32_t carry_last = -1;          // the last position with e == 0 in the segments so far (uniform)
  unsigned long long bits_sum = 0;  // this thread's token bits (size kernel)
  unsigned long long a1 = 0, a2 = 0;  // this thread's share of the sums of d[i] and of (n - i) d[i]
  // the encode kernel's stream position (uniform): the aligned dword the buffer's word 0 goes to, the bits the buffer holds, the bytes of the chunk's
  // first dword that belong to the chunk in front
  uint8_t* out_at = nullptr;
  uint32_t held = 0u, head = 0u;
  if (ENCODE) {
    head = (uint32_t)(reinterpret_cast<uintptr_t>(chunk) & 3u);
    out_at = chunk - head;
    for (uint32_t w = tid; w < ZIPS_OUT_DWORDS; w += EXR_ZIPS_BLOCK) S.out[w] = 0u;
    __syncthreads();
    if (tid == 0u) {  // the prefix and the 19 bits in front of the first token, behind `head` bytes that stay zero here and are never stored
      const unsigned long long pieces[3] = {y, size, ZIPS_HEAD};
      const uint32_t lengths[3] = {32u, 32u, ZIPS_HEAD_BITS};
      uint32_t at = 8u * head;
      for (int k = 0; k < 3; ++k) {
        const unsigned long long v = pieces[k] << (at & 31u);
        S.out[at >> 5] |= (uint32_t)v;
        S.out[(at >> 5) + 1u] |= (uint32_t)(v >> 32);
        at += lengths[k];
      }
    }
    held = 8u * head + 64u + ZIPS_HEAD_BITS;
    __syncthreads();
  }
  // the stream's complete dwords leave; the partial one moves to the front.  last: the stream ends here, on a byte: its last bytes leave too
  auto flush = [&](bool last) {
    const uint32_t whole = held >> 5, rest_bytes = last ? (held & 31u) >> 3 : 0u;
    const uint32_t rest = S.out[whole];
    for (uint32_t w = tid; w < whole; w += EXR_ZIPS_BLOCK) store_chunk_dword(out_at, w, S.out[w], w == 0u ? head : 0u, 4u);
    if (tid == 0u && rest_bytes > (whole == 0u ? head : 0u)) store_chunk_dword(out_at, whole, rest, whole == 0u ? head : 0u, rest_bytes);
    __syncthreads();
    for (uint32_t w = tid; w <= whole; w += EXR_ZIPS_BLOCK) S.out[w] = w == 0u ? rest : 0u;
    if (whole) head = 0u;
    out_at += 4u * (size_t)whole;
    held &= 31u;
    __syncthreads();
  };

  for (uint32_t seg = 0; seg < n_segments; ++seg) {
    const int32_t a = (int32_t)(seg * EXR_ZIPS_SEGMENT);
    // d of the positions a - 4 .. a + SEGMENT + 258 + (up to 3), four per dword; positions outside the row read as 0
    for (uint32_t q = tid; q < ZIPS_D_DWORDS; q += EXR_ZIPS_BLOCK) {
      const int32_t p0 = a - 4 + 4 * (int32_t)q;
      uint32_t prev = (p0 >= 1 && p0 <= (int32_t)n) ? raw[zips_raw_index((uint32_t)p0 - 1u, n)] : 0u, word = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int32_t p = p0 + j;
        if (p >= 0 && p < (int32_t)n) {
          const uint32_t t = raw[zips_raw_index((uint32_t)p, n)];
          word |= (p == 0 ? t : ((t - prev + 128u) & 255u)) << (8 * j);
          prev = t;
        }
      }
      S.d[q] = word;
    }
    if (tid == 0u) S.halo_zero = ZIPS_NONE;
    __syncthreads();

    // the strip: 16 bytes of d and the two in front of them; e of its positions as a mask
    const int32_t s0 = a + (int32_t)(tid * EXR_ZIPS_STRIP);
    uint32_t dw[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) dw[k] = S.d[tid * 4u + (uint32_t)k];  // dw[0]: the positions s0 - 4 .. s0 - 1
    auto strip_d = [&](int j) { return (dw[(j + 4) >> 2] >> (8 * ((j + 4) & 3))) & 255u; };  // j = -2 .. 15
    uint32_t e_mask = 0u;
#pragma unroll
    for (int j = 0; j < (int)EXR_ZIPS_STRIP; ++j) {
      const int32_t p = s0 + j;
      if (p >= 2 && p < (int32_t)n && strip_d(j) == strip_d(j - 2)) e_mask |= 1u << j;
    }
    const uint32_t zero_mask = ~e_mask & 0xffffu;
    // the look-ahead behind the segment: its first position with e == 0 (a position behind the row's end counts: the interval ends there)
    for (uint32_t j = tid; j < ZIPS_MAX_MATCH; j += EXR_ZIPS_BLOCK) {
      const int32_t rel = (int32_t)(EXR_ZIPS_SEGMENT + j), p = a + rel;
      if (p >= (int32_t)n || d_byte(S, rel) != d_byte(S, rel - 2)) atomicMin(&S.halo_zero, (uint32_t)p);
    }
    // the last e == 0 position at or before the strip's end (inclusive maximum), the first one from the strip's start on (inclusive minimum, from behind)
    int32_t last = zero_mask ? s0 + (31 - (int32_t)__clz((int)zero_mask)) : -1;
    uint32_t next = zero_mask ? (uint32_t)s0 + (uint32_t)(__ffs((int)zero_mask) - 1) : ZIPS_NONE;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
      const int32_t up = __shfl_up(last, o);
      const uint32_t down = __shfl_down(next, o);
      if (lane >= o) last = max(last, up);
      if (lane + o < 64u) next = min(next, down);
    }
    if (lane == 63u) S.wave_last[wave] = last;
    if (lane == 0u) S.wave_next[wave] = next;
    int32_t before = __shfl_up(last, 1);        // ... of the strips in front of this one, in this wave
    uint32_t behind = __shfl_down(next, 1);     // ... of the strips behind it
    if (lane == 0u) before = -1;
    if (lane == 63u) behind = ZIPS_NONE;
    __syncthreads();
    before = max(before, carry_last);
    behind = min(behind, S.halo_zero);
#pragma unroll
    for (uint32_t w = 0; w < EXR_ZIPS_WAVES; ++w) {
      if (w < wave) before = max(before, S.wave_last[w]);
      if (w > wave) behind = min(behind, S.wave_next[w]);
    }
    carry_last = max(carry_last, max(max(S.wave_last[0], S.wave_last[1]), max(S.wave_last[2], S.wave_last[3])));
    static_assert(EXR_ZIPS_WAVES == 4u, "the maximum above names four waves");

    // the strip's tokens
    uint32_t token[EXR_ZIPS_STRIP];  // the bits as written | their number << 24
    uint32_t strip_bits = 0u;
#pragma unroll
    for (int j = 0; j < (int)EXR_ZIPS_STRIP; ++j) {
      const int32_t p = s0 + j;
      const uint32_t d = strip_d(j);
      uint32_t r = 0u, f = 0u, nb = 0u, code = 0u;
      const bool e = (e_mask >> j) & 1u;
      if (e) {
        const uint32_t lower = zero_mask & ((1u << j) - 1u), upper = zero_mask >> (j + 1);
        const int32_t zero_before = lower ? s0 + (31 - (int32_t)__clz((int)lower)) : before;  // (an e == 1 position has one: e[0] == e[1] == 0)
        const uint32_t zero_behind = upper ? (uint32_t)p + (uint32_t)__ffs((int)upper) : behind;
        r = (uint32_t)(p - zero_before - 1) % ZIPS_MAX_MATCH;
        f = min(zero_behind - (uint32_t)p, ZIPS_MAX_MATCH);  // (ZIPS_NONE: further than the look-ahead)
      }
      if (p < (int32_t)n) {
        code = zips_token(d, e, r, f, &nb);
        a1 += d;
        a2 += (unsigned long long)(n - (uint32_t)p) * d;
      }
      token[j] = code | (nb << 24);
      strip_bits += nb;
    }
    if (!ENCODE) {
      bits_sum += strip_bits;
      __syncthreads();  // (the next segment overwrites d and the waves' figures)
      continue;
    }
    // where the strip's bits start: the sum over the strips in front of it, behind the bits the buffer holds
    uint32_t incl = strip_bits;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == 63u) S.wave_bits[wave] = incl;
    __syncthreads();
    uint32_t at = held + incl - strip_bits, segment_bits = 0u;
#pragma unroll
    for (uint32_t w = 0; w < EXR_ZIPS_WAVES; ++w) {
      if (w < wave) at += S.wave_bits[w];
      segment_bits += S.wave_bits[w];
    }
    unsigned long long acc = 0;
    uint32_t word = at >> 5, cnt = at & 31u;
#pragma unroll
    for (int j = 0; j < (int)EXR_ZIPS_STRIP; ++j) {
      acc |= (unsigned long long)(token[j] & 0xffffffu) << cnt;
      cnt += token[j] >> 24;
      if (cnt >= 32u) {
        atomicOr(&S.out[word++], (uint32_t)acc);
        acc >>= 32;
        cnt -= 32u;
      }
    }
    if (cnt) atomicOr(&S.out[word], (uint32_t)acc);
    held += segment_bits;
    __syncthreads();
    flush(false);
  }

  if (!ENCODE) {
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) bits_sum += __shfl_down(bits_sum, o);
    if (lane == 0u) S.sums[0][wave] = bits_sum;
    __syncthreads();
    return S.sums[0][0] + S.sums[0][1] + S.sums[0][2] + S.sums[0][3];
  }
  // the end of the block, zero bits to the byte, Adler-32 big-endian
#pragma unroll
  for (uint32_t o = 32; o; o >>= 1) a1 += __shfl_down(a1, o), a2 += __shfl_down(a2, o);
  if (lane == 0u) S.sums[1][wave] = a1, S.sums[2][wave] = a2;
  __syncthreads();
  held = (held + ZIPS_EOB_BITS + 7u) & ~7u;
  if (tid == 0u) {
    const uint32_t s1 = (uint32_t)((1u + S.sums[1][0] + S.sums[1][1] + S.sums[1][2] + S.sums[1][3]) % ZIPS_ADLER_MOD);
    const uint32_t s2 = (uint32_t)((n + S.sums[2][0] + S.sums[2][1] + S.sums[2][2] + S.sums[2][3]) % ZIPS_ADLER_MOD);
    const uint32_t adler = (s2 << 16) | s1;
    const unsigned long long v = (unsigned long long)__builtin_bswap32(adler) << (held & 31u);
    S.out[held >> 5] |= (uint32_t)v;
    S.out[(held >> 5) + 1u] |= (uint32_t)(v >> 32);
  }
  held += 32u;
  __syncthreads();
  flush(true);
  return 0;
}

}  // namespace

__global__ void __launch_bounds__(EXR_ZIPS_BLOCK) zips_size_kernel(ZipsLaunch L) {
  __shared__ ZipsShared S;
  const uint32_t y = blockIdx.x, n = L.row_bytes;
  const uint8_t* raw = L.body + (size_t)y * (8u + (size_t)n) + 8u;
  const unsigned long long token_bits = zips_row<false>(S, raw, n, y, 0u, nullptr);
  if (threadIdx.x == 0u) {
    const uint64_t z = zips_stream_bytes(token_bits);
    L.sizes[y] = z >= n ? n : (uint32_t)z;
  }
}

// sizes -> the offset table (absolute file offsets: the tail follows attr_bytes of attributes) and the tail's length
__global__ void __launch_bounds__(EXR_ZIPS_BLOCK) zips_scan_kernel(ZipsLaunch L) {
  __shared__ unsigned long long part[EXR_ZIPS_BLOCK];
  const uint32_t tid = threadIdx.x, per = (L.height + EXR_ZIPS_BLOCK - 1u) / EXR_ZIPS_BLOCK;
  const uint32_t y0 = min(tid * per, L.height), y1 = min(y0 + per, L.height);
  unsigned long long sum = 0;
  for (uint32_t y = y0; y < y1; ++y) sum += 8u + L.sizes[y];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0u) {
    unsigned long long run = 8ull * L.height;
    for (uint32_t t = 0; t < EXR_ZIPS_BLOCK; ++t) {
      const unsigned long long s = part[t];
      part[t] = run;
      run += s;
    }
    *L.written = run;
  }
  __syncthreads();
  unsigned long long at = part[tid];
  unsigned long long* table = reinterpret_cast<unsigned long long*>(L.tail);
  for (uint32_t y = y0; y < y1; ++y) {
    table[y] = L.attr_bytes + at;
    at += 8u + L.sizes[y];
  }
}

__global__ void __launch_bounds__(EXR_ZIPS_BLOCK) zips_encode_kernel(ZipsLaunch L) {
  __shared__ ZipsShared S;
  const uint32_t y = blockIdx.x, n = L.row_bytes, size = L.sizes[y];
  const uint8_t* row = L.body + (size_t)y * (8u + (size_t)n);  // its prefix included
  uint8_t* chunk = L.tail + (reinterpret_cast<const unsigned long long*>(L.tail)[y] - L.attr_bytes);
  if (size != n) {
    zips_row<true>(S, row + 8u, n, y, size, chunk);
    return;
  }
  // stored raw: the body's chunk as it is, dword by dword of the destination
  const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(chunk) & 3u), total = 8u + n;
  uint8_t* aligned = chunk - head;
  const uint32_t dwords = (head + total + 3u) / 4u;
  for (uint32_t w = threadIdx.x; w < dwords; w += EXR_ZIPS_BLOCK) {
    const uint32_t first = 4u * w;  // the dword's first byte, counted from `aligned`
    const uint32_t lo = first < head ? head - first : 0u, hi = min(4u, head + total - first);
    uint32_t v = 0u;
    for (uint32_t b = lo; b < hi; ++b) v |= (uint32_t)row[first + b - head] << (8u * b);
    store_chunk_dword(aligned, w, v, lo, hi);
  }
}

hipError_t launch_exr_zips_size(const ZipsLaunch& L, hipStream_t st) {
  if (L.height == 0u || L.row_bytes == 0u || (L.row_bytes & 1u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(zips_size_kernel, dim3(L.height), dim3(EXR_ZIPS_BLOCK), 0, st, L);
  return hipGetLastError();
}
hipError_t launch_exr_zips_scan(const ZipsLaunch& L, hipStream_t st) {
  hipLaunchKernelGGL(zips_scan_kernel, dim3(1), dim3(EXR_ZIPS_BLOCK), 0, st, L);
  return hipGetLastError();
}
hipError_t launch_exr_zips_encode(const ZipsLaunch& L, hipStream_t st) {
  hipLaunchKernelGGL(zips_encode_kernel, dim3(L.height), dim3(EXR_ZIPS_BLOCK), 0, st, L);
  return hipGetLastError();
}

}  // namespace rene
