// kernels_state.hip -- the checkpoint of a render job (rene_save_state / rene_restore_state, include/rene_hip.h): one more pass over the eight frame
// chains (device_scene.h, CHAINS), and its inverse.  Both move bits and add integers; no float is ever computed with, so NaN payloads, -0.0 and
// denormals travel as they are whatever the unit's floating-point flags.
//
//   one workgroup of PASS_BLOCK = 256 threads per OWNED tile of a chunk, as in chain_pass.h.  The chains hold the tile's 24 planes (chain, layer) as
//   1024 16-byte records {r, g, b, version} in SLOT order (8 x 8 sub-blocks); the state's payload holds them as [32 dy][32 dx][3] floats, row-major.
//
// state_pack_kernel, per plane: thread j reads the records of slots j, j + 256, j + 512, j + 768 -- consecutive lanes, consecutive 16-byte records --
// and writes their three floats to the pixel's place in an LDS image of the plane; after the barrier the workgroup reads that image linearly, 16 bytes
// per lane, and stores it to the chunk buffer: whole rows, not the 8-pixel pieces of the sub-blocks.  The LDS image is double-buffered, so a plane
// costs ONE barrier: the plane after next is written only behind the barrier that ends the next, which no thread reaches before it has read this one.
//   The LDS row is STATE_ROW = 120 floats, not 96.  ds_write_b32 / ds_read_b32 bank a dword address modulo 32 within a 32-lane half; a half covers
//   the pixels dx = 0 .. 7 of rows dy = 0 .. 3 of one sub-block, at dword 120 dy + 3 dx (+ channel): 3 dx + 24 dy takes 32 distinct values modulo 32,
//   so by that banking rule the scattered side is conflict-free (reasoning from the rule; no counter run has confirmed it).  120 floats are a multiple of 16 bytes, so the linear side is ds_read_b128 / ds_write_b128 on consecutive slots.
// The tile's checksum -- c0 = sum of the payload dwords w_i, c1 = sum of (i + 1) w_i, mod 2^32 -- is taken from the dwords on their way out, reduced in
// the fixed order of chain_pass.h (tile_reduce; integer sums: any order gives the same) and stored with one 8-byte store per tile.  No atomics.
//
// state_unpack_kernel is the inverse: the payload read linearly into the LDS image (and summed into c0 / c1 as it ARRIVED on the device, for the host to
// compare with the table), then every thread builds the records of its four slots: {r, g, b, 0} -- the version word rene_reset leaves -- inside the
// image, a zero record outside.
//
// Bounds: the grid is exactly the chunk's tiles; owned tile k = first_owned + blockIdx.x < n_slots / 1024 is the host's to guarantee (launch_state
// checks it), and the chunk buffer holds STATE_TILE_DWORDS dwords per tile of the chunk.
#include <hip/hip_runtime.h>

#include "chain_pass.h"

namespace rene {

constexpr uint32_t STATE_ROW = 120;                                                // LDS row stride in dwords (above)
constexpr uint32_t STATE_PLANES = CHAINS * 3u;                                     // (chain, layer)
constexpr uint32_t STATE_PLANE_DWORDS = RENE_TILE_SIZE * RENE_TILE_SIZE * 3u;      // 3072
constexpr uint32_t STATE_PLANE_VEC = STATE_PLANE_DWORDS / 4u;                      // 768 16-byte pieces, 24 per row
constexpr uint32_t STATE_VEC_PER_THREAD = STATE_PLANE_VEC / PASS_BLOCK;            // 3
static_assert(STATE_PLANES * STATE_PLANE_DWORDS == STATE_TILE_DWORDS, "a tile's payload is its 24 planes");
static_assert(STATE_PLANE_VEC % PASS_BLOCK == 0 && STATE_ROW % 4u == 0 && STATE_ROW >= RENE_TILE_SIZE * 3u, "the linear side moves 16 bytes per lane");

// piece v (0 .. 767) of a plane's row-major image -> its dword in the LDS image
__device__ __forceinline__ uint32_t state_lds_vec(uint32_t v) { return (v / 24u) * STATE_ROW + (v % 24u) * 4u; }

__device__ __forceinline__ void state_sum(TileSums<0, 2>& s, uint32_t i, const uint4& w) {  // the dwords i .. i + 3 of the tile's payload
  s.u[0] += (w.x + w.y) + (w.z + w.w);
  s.u[1] += (i + 1u) * w.x + (i + 2u) * w.y + (i + 3u) * w.z + (i + 4u) * w.w;
}

__global__ void __launch_bounds__(PASS_BLOCK) state_pack_kernel(const uint4* __restrict__ chains, uint4* __restrict__ chunk, uint2* __restrict__ sums, StateLaunch L) {
  __shared__ __attribute__((aligned(16))) uint32_t s_img[2][RENE_TILE_SIZE * STATE_ROW];
  const uint32_t k = L.first_owned + blockIdx.x;
  const uint2 o = owned_tile_origin(L.grid, k);
  const size_t n_slots = L.grid.n_slots;
  const uint4* src = chains + (size_t)k * TILE_SLOTS + threadIdx.x;
  uint4* dst = chunk + (size_t)blockIdx.x * (STATE_TILE_DWORDS / 4u) + threadIdx.x;
  uint32_t at[PASS_PER_THREAD];  // where the thread's four pixels go in the LDS image; outside the image: ~0
#pragma unroll
  for (uint32_t q = 0; q < PASS_PER_THREAD; ++q) {
    const uint2 d = slot_pixel(threadIdx.x + q * PASS_BLOCK);
    at[q] = (o.x + d.x < L.grid.width && o.y + d.y < L.grid.height) ? 1u : 0u;
    at[q] |= (d.y * STATE_ROW + d.x * 3u) << 1;
  }
  TileSums<0, 2> s{};
  for (uint32_t p = 0; p < STATE_PLANES; ++p) {
    uint32_t* img = s_img[p & 1u];
    uint4 rec[PASS_PER_THREAD];
#pragma unroll
    for (uint32_t q = 0; q < PASS_PER_THREAD; ++q) rec[q] = src[(size_t)p * n_slots + q * PASS_BLOCK];
#pragma unroll
    for (uint32_t q = 0; q < PASS_PER_THREAD; ++q) {
      const bool inside = (at[q] & 1u) != 0;  // a ragged tile's pixels outside the image are zero in the payload
      uint32_t* px = img + (at[q] >> 1);
      px[0] = inside ? rec[q].x : 0u;
      px[1] = inside ? rec[q].y : 0u;
      px[2] = inside ? rec[q].z : 0u;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < STATE_VEC_PER_THREAD; ++j) {
      const uint32_t v = threadIdx.x + j * PASS_BLOCK;
      const uint4 w = *reinterpret_cast<const uint4*>(img + state_lds_vec(v));
      dst[p * STATE_PLANE_VEC + j * PASS_BLOCK] = w;
      state_sum(s, p * STATE_PLANE_DWORDS + v * 4u, w);
    }
  }
  if (tile_reduce(s)) sums[k] = make_uint2(s.u[0], s.u[1]);  // one store of the tile's checksum
}

__global__ void __launch_bounds__(PASS_BLOCK) state_unpack_kernel(uint4* __restrict__ chains, const uint4* __restrict__ chunk, uint2* __restrict__ sums, StateLaunch L) {
  __shared__ __attribute__((aligned(16))) uint32_t s_img[2][RENE_TILE_SIZE * STATE_ROW];
  const uint32_t k = L.first_owned + blockIdx.x;
  const uint2 o = owned_tile_origin(L.grid, k);
  const size_t n_slots = L.grid.n_slots;
  uint4* dst = chains + (size_t)k * TILE_SLOTS + threadIdx.x;
  const uint4* src = chunk + (size_t)blockIdx.x * (STATE_TILE_DWORDS / 4u) + threadIdx.x;
  uint32_t at[PASS_PER_THREAD];
#pragma unroll
  for (uint32_t q = 0; q < PASS_PER_THREAD; ++q) {
    const uint2 d = slot_pixel(threadIdx.x + q * PASS_BLOCK);
    at[q] = (o.x + d.x < L.grid.width && o.y + d.y < L.grid.height) ? 1u : 0u;
    at[q] |= (d.y * STATE_ROW + d.x * 3u) << 1;
  }
  TileSums<0, 2> s{};
  for (uint32_t p = 0; p < STATE_PLANES; ++p) {
    uint32_t* img = s_img[p & 1u];
#pragma unroll
    for (uint32_t j = 0; j < STATE_VEC_PER_THREAD; ++j) {
      const uint32_t v = threadIdx.x + j * PASS_BLOCK;
      const uint4 w = src[p * STATE_PLANE_VEC + j * PASS_BLOCK];
      *reinterpret_cast<uint4*>(img + state_lds_vec(v)) = w;
      state_sum(s, p * STATE_PLANE_DWORDS + v * 4u, w);  // what arrived, whether or not it is kept
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < PASS_PER_THREAD; ++q) {
      const bool inside = (at[q] & 1u) != 0;  // slots outside the image are zero, as rene_reset leaves them
      const uint32_t* px = img + (at[q] >> 1);
      dst[(size_t)p * n_slots + q * PASS_BLOCK] = inside ? make_uint4(px[0], px[1], px[2], 0u) : make_uint4(0u, 0u, 0u, 0u);  // version 0
    }
  }
  if (tile_reduce(s)) sums[k] = make_uint2(s.u[0], s.u[1]);
}

hipError_t launch_state(float* chains, void* chunk, void* sums, const StateLaunch& L, bool unpack, hipStream_t st) {
  if (L.n_tiles == 0) return hipSuccess;
  if ((uint64_t)L.first_owned + L.n_tiles > L.grid.n_slots / TILE_SLOTS) return hipErrorInvalidValue;  // the chunk's tiles are owned tiles
  if (unpack)
    hipLaunchKernelGGL(state_unpack_kernel, dim3(L.n_tiles), dim3(PASS_BLOCK), 0, st, reinterpret_cast<uint4*>(chains), static_cast<const uint4*>(chunk), static_cast<uint2*>(sums), L);
  else
    hipLaunchKernelGGL(state_pack_kernel, dim3(L.n_tiles), dim3(PASS_BLOCK), 0, st, reinterpret_cast<const uint4*>(chains), static_cast<uint4*>(chunk), static_cast<uint2*>(sums), L);
  return hipGetLastError();
}

}  // namespace rene
