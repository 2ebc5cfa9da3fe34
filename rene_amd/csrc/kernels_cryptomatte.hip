// kernels_cryptomatte.hip -- the body of a Cryptomatte file on the device (rene_output_cryptomatte, include/rene_hip.h): up to three layers' 64-byte
// geometry records and the hashes of their names in, the scan-line chunks of an uncompressed OpenEXR file out, in their final byte layout -- bit for
// bit the bytes of the host's rene_cryptomatte_body_host.
//
//   The body: row y is one chunk at y * (8 + W * 32 * layers) -- int32 y, int32 W * 32 * layers, then one row of W dwords per channel, the channels
//   in the order of their names' bytes.  A layer has eight FLOAT channels, <L>00.A .B .G .R and <L>01.A .B .G .R; R and B hold the ids of an even
//   and an odd rank, G and A their coverages.  Where the rows of a layer lie in the chunk is the host's to say (row_index: the names of two layers
//   may interleave).
//
//   Mapping: exr_kernel's -- the grid's y is the row and a lane is one pixel of it, so 64 consecutive lanes store 64 consecutive dwords of one
//   channel row.  Every channel takes 4 bytes: a chunk is 8 + 32 * layers * W bytes, a multiple of 4 for every W, and every channel row starts on
//   a dword of the 4-byte aligned destination -- the two-halves store of kernels_exr.hip has no case here, every store is one aligned dword.
//   A tile shard writes the bytes of its own tiles' pixels, and the lane of x = 0 the row's prefix where the shard owns a tile of that tile row.
//   The loads come first: per layer n, the four ids and the four counts of the record, then up to four look-ups of an id's hash -- a gather into a
//   table of a few KB that stays in the cache.  Merge and order are a fixed network on four (count, key) pairs in registers: six compares to
//   merge, five compare-exchanges to sort, no loop over the data, no scratch.  No LDS, no atomics.  Nothing here writes the records.
//
// The specification fixes the one fp32 operation, count / n: this unit is built with ROBUSTFLAGS (Makefile) -- the correctly rounded division,
// denormals kept.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rene {

constexpr uint32_t CRYPTOMATTE_BLOCK = 256;

namespace {

// one slot or rank: the sample count and the hash of the id's name
struct Matte {
  uint32_t count, key;
};
// a before b in the file: the larger count, then the smaller key
__device__ __forceinline__ bool before(const Matte& a, const Matte& b) { return a.count > b.count || (a.count == b.count && a.key < b.key); }
__device__ __forceinline__ void order(Matte& a, Matte& b) {
  const bool swap = before(b, a);
  const Matte lo = swap ? b : a, hi = swap ? a : b;
  a = lo, b = hi;
}

}  // namespace

__global__ void __launch_bounds__(CRYPTOMATTE_BLOCK) cryptomatte_kernel(CryptomatteLaunch L) {
  const uint32_t y = blockIdx.y, x = blockIdx.x * CRYPTOMATTE_BLOCK + threadIdx.x;
  if (x >= L.width) return;
  const uint32_t row_data = L.width * 32u * L.n_layers;  // (at most 16384 x 96)
  uint8_t* const row = static_cast<uint8_t*>(L.dst) + (size_t)y * (8u + (size_t)row_data);
  const uint32_t tile = (y / RENE_TILE_SIZE) * L.tiles_x + x / RENE_TILE_SIZE;
  bool prefix = x == 0u;
  if (L.shard_count > 1u) {
    if (prefix) {  // does the shard own one of the tiles tile .. tile + tiles_x - 1 of this tile row?
      const uint32_t first = tile % L.shard_count;
      const uint32_t d = (L.shard_rank + L.shard_count - first) % L.shard_count;
      prefix = d < L.tiles_x;
    }
    uint32_t rem = tile - __umulhi(tile, L.shard_inv) * L.shard_count;  // mulhi(tile, floor(2^32 / shard_count)) is the quotient or one less
    rem -= rem >= L.shard_count ? L.shard_count : 0u;
    if (prefix) reinterpret_cast<uint32_t*>(row)[0] = y, reinterpret_cast<uint32_t*>(row)[1] = row_data;
    if (rem != L.shard_rank) return;
  } else if (prefix) {
    reinterpret_cast<uint32_t*>(row)[0] = y, reinterpret_cast<uint32_t*>(row)[1] = row_data;
  }
  // the loads, all of them ahead of the first use: the records ...
  const size_t p = (size_t)y * L.width + x;
  uint32_t n[CRYPTOMATTE_LAYERS];
  uint4 id[CRYPTOMATTE_LAYERS], count[CRYPTOMATTE_LAYERS];
#pragma unroll
  for (uint32_t l = 0; l < CRYPTOMATTE_LAYERS; ++l) {
    n[l] = 0u, id[l] = count[l] = make_uint4(0u, 0u, 0u, 0u);
    if (l < L.n_layers) {
      const uint4* rec = reinterpret_cast<const uint4*>(L.records[l]) + 4u * p;  // {depth_sum, depth_min, hits, n} {position_sum, other} {id} {count}
      n[l] = reinterpret_cast<const uint32_t*>(rec)[3];
      id[l] = rec[2], count[l] = rec[3];
    }
  }
  // ... then the hashes of the slots that count (rule 2: count > 0 and an id inside the table; any other slot is dropped as count 0)
  Matte m[CRYPTOMATTE_LAYERS][4];
#pragma unroll
  for (uint32_t l = 0; l < CRYPTOMATTE_LAYERS; ++l) {
    const uint32_t ids[4] = {id[l].x, id[l].y, id[l].z, id[l].w}, counts[4] = {count[l].x, count[l].y, count[l].z, count[l].w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool counts_k = l < L.n_layers && counts[k] > 0u && ids[k] < L.n_names[l];
      m[l][k].count = counts_k ? counts[k] : 0u;
      m[l][k].key = counts_k ? L.hashes[l][ids[k]] : 0u;
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // (nothing that consumes a load is scheduled up between the loads: it would wait for them one by one)

#pragma unroll
  for (uint32_t l = 0; l < CRYPTOMATTE_LAYERS; ++l) {
    if (l >= L.n_layers) break;
    Matte* s = m[l];
    // rule 3: a slot whose key is a lower counting slot's adds its count to that slot and is dropped
#pragma unroll
    for (int k = 1; k < 4; ++k) {
#pragma unroll
      for (int j = 0; j < k; ++j) {
        const bool same = s[k].count > 0u && s[j].count > 0u && s[k].key == s[j].key;
        s[j].count += same ? s[k].count : 0u;
        s[k].count = same ? 0u : s[k].count;
      }
    }
    // rule 4: the sorting network of four elements; a dropped slot (count 0) ends behind every counting one
    order(s[0], s[1]), order(s[2], s[3]), order(s[0], s[2]), order(s[1], s[3]), order(s[1], s[2]);
    // rule 5, and rule 1 for a pixel no pass has filled
    const float n_f = (float)n[l];
    uint32_t ids[4], cov[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool used = n[l] != 0u && s[r].count > 0u;
      ids[r] = used ? s[r].key : 0u;
      cov[r] = used ? __float_as_uint((float)s[r].count / n_f) : 0u;
    }
    // a level's A B G R = the odd rank's coverage and id, the even rank's coverage and id
    const uint32_t value[8] = {cov[1], ids[1], cov[0], ids[0], cov[3], ids[3], cov[2], ids[2]};
#pragma unroll
    for (int c = 0; c < 8; ++c) reinterpret_cast<uint32_t*>(row + 8u + (size_t)L.row_index[l][c] * 4u * L.width)[x] = value[c];
  }
}

hipError_t launch_cryptomatte(const CryptomatteLaunch& L, hipStream_t st) {
  if (L.width == 0 || L.height == 0) return hipSuccess;
  if (L.height > 65535u || L.n_layers < 1u || L.n_layers > CRYPTOMATTE_LAYERS) return hipErrorInvalidValue;
  for (uint32_t l = 0; l < L.n_layers; ++l)
    for (int c = 0; c < 8; ++c)
      if (L.row_index[l][c] >= 8u * L.n_layers) return hipErrorInvalidValue;  // (a row outside the chunk)
  const dim3 grid((L.width + CRYPTOMATTE_BLOCK - 1u) / CRYPTOMATTE_BLOCK, L.height), block(CRYPTOMATTE_BLOCK);
  hipLaunchKernelGGL(cryptomatte_kernel, grid, block, 0, st, L);
  return hipGetLastError();
}

}  // namespace rene
