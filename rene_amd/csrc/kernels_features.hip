// kernels_features.hip -- the denoiser hand-off (rene_export_features, include/rene_hip.h): per owned pixel the MEANS a denoiser or a network wants --
// radiance, first-hit albedo and normal, the variance of the mean's luminance, the two half-images of the even and of the odd frame chains, the
// frame count -- written in one pass over the chains as a tightly packed tensor, [C][H][W] or [H][W][C], fp32 or fp16.
//
//   one workgroup of 256 threads per OWNED tile k, its origin and its own chain counts under adaptive sampling from chain_pass.h
//   (owned_tile_origin, tile_chain_counts).  The threads are mapped PIXEL-MAJOR inside the tile, a mapping of this kernel's own: in step q (0..3)
//   thread j takes the pixel (j & 31, 8 q + (j >> 5)), so a wave covers two rows of 32 pixels.  A tile's slots are ordered in 8 x 8 sub-blocks (device_scene.h): a row of 32 pixels is four runs of
//   eight consecutive slots, and a wave's 16-byte chain loads come in 128-byte runs.  The guide layers are read from the resolved image, which is
//   pixel-major already (512-byte runs).
//
//   The write side: a planar tensor ([C][H][W]) takes the pixel-major mapping as it is -- 32 consecutive lanes store 32 consecutive elements of a
//   plane row.  An interleaved tensor ([H][W][C]) would have every lane store C elements of its own pixel, a stride of C elements between lanes;
//   instead the eight rows of a step are staged in LDS as they lie in memory (a tile row's pixels are one contiguous run of 32 C elements) and
//   copied out by the waves, consecutive lanes to consecutive elements.
//
//   The feature mask is a kernel argument (wave-uniform): a channel that is not requested costs neither its loads nor its stores; the channel
//   positions follow from the mask in bit order.  Format and layout are template parameters.
//
// The specification fixes every fp32 operation and its order: this unit is compiled with ROBUSTFLAGS (Makefile) -- no fused multiply-add, the
// correctly rounded division, denormals kept -- and is held bit for bit to tests/features_reference.py; COLOR, ALBEDO and NORMAL are bit for bit
// rene_download_mean's.  No atomics.  Nothing here writes the accumulation state.
#include <hip/hip_runtime.h>

#include "chain_pass.h"
#include "half_element.h"  // to_element: the fp32 -> fp16 rule, shared with kernels_exr.hip

namespace rene {

namespace {

constexpr uint32_t FEAT_BLOCK = PASS_BLOCK, FEAT_STEPS = PASS_PER_THREAD, FEAT_STEP_ROWS = FEAT_BLOCK / RENE_TILE_SIZE, FEAT_WAVES = PASS_WAVES;
constexpr uint32_t FEAT_MAX_CHANNELS = 17;

// the slot of the tile's pixel (px, py): tile_slot() of device_scene.h, written with sums.  (With tile_slot() itself, whose terms are joined by `|`,
// the planar fp32 instantiation takes 72 VGPRs where this form takes 70, the bound of tests/test_features_resources.py; that the two agree on every
// pixel of a tile is checked here, at compile time.)
constexpr uint32_t pixel_slot(uint32_t px, uint32_t py) { return (((py >> 3) * 4u + (px >> 3)) << 6) + ((py & 7u) << 3) + (px & 7u); }
constexpr bool pixel_slot_is_tile_slot() {
  for (uint32_t py = 0; py < RENE_TILE_SIZE; ++py)
    for (uint32_t px = 0; px < RENE_TILE_SIZE; ++px)
      if (pixel_slot(px, py) != tile_slot(px, py)) return false;
  return true;
}
static_assert(pixel_slot_is_tile_slot(), "pixel_slot and tile_slot (device_scene.h) disagree");

}  // namespace

template <class T, bool HWC>
__global__ void __launch_bounds__(FEAT_BLOCK) features_kernel(const float4* __restrict__ chains, const float4* __restrict__ image, T* __restrict__ dst, FeatureLaunch L) {
  __shared__ T s_stage[HWC ? FEAT_BLOCK * FEAT_MAX_CHANNELS : 1];  // [8 rows][32 pixels][C]: the rows of a step as they lie in an [H][W][C] tensor
  // owned tile (the grid is exactly the owned tiles: k * 1024 + 1023 < n_slots).  A tile row of a plane of 2-byte elements is 64 bytes, half a
  // 128-byte cache line whose other half belongs to the next tile; consecutive workgroups go to different XCDs, each with an L2 of its own, and
  // the line would leave two of them half written.  So within every full group of 16 workgroups, b and b + 8 -- the same XCD where workgroups
  // are dealt round-robin to eight of them, and in flight together -- take the tiles 2m and 2m + 1.  (A permutation of the tiles whatever the
  // placement is: nothing but the speed depends on it.)
  const uint32_t b = blockIdx.x, b16 = b & ~15u;
  const uint32_t k = b16 + 16u <= gridDim.x ? b16 + 2u * (b & 7u) + ((b >> 3) & 1u) : b;
  uint32_t cn[CHAINS];
  tile_chain_counts(L.counts, k, cn);
  uint32_t n_total = 0, kk = 0, n_half[2] = {0, 0};  // N_t, the chains that have received frames, the frames of the even and of the odd chains
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    n_total += cn[g];
    kk += cn[g] ? 1u : 0u;
    n_half[g & 1u] += cn[g];
  }
  const float n_total_f = (float)n_total, half_f[2] = {(float)n_half[0], (float)n_half[1]};
  float nf[CHAINS], share[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    nf[g] = (float)cn[g];
    share[g] = n_total ? nf[g] / n_total_f : 0.0f;
  }
  const uint32_t F = L.features, C = L.channels;
  const bool want_chains = n_total != 0 && (F & (RENE_FEATURE_COLOR | RENE_FEATURE_VARIANCE | RENE_FEATURE_HALF_A | RENE_FEATURE_HALF_B)) != 0;
  const uint2 o = owned_tile_origin(L.grid, k);
  const uint32_t x0 = o.x, y0 = o.y;
  const uint32_t row_px = x0 < L.grid.width ? min(RENE_TILE_SIZE, L.grid.width - x0) : 0u;  // the tile's pixels per row inside the image
  const size_t n4 = (size_t)3 * L.grid.n_slots, n_px = (size_t)L.grid.width * L.grid.height;
  const uint32_t px = threadIdx.x & 31u, x = x0 + px;
#pragma unroll
  for (uint32_t q = 0; q < FEAT_STEPS; ++q) {
    const uint32_t py = q * FEAT_STEP_ROWS + (threadIdx.x >> 5), y = y0 + py;
    const uint32_t slot = pixel_slot(px, py);
    const bool inside = x < L.grid.width && y < L.grid.height;
    // a ragged tile's slots outside the image exist (and hold zeros): their loads are in bounds, nothing is written for them
    float4 c[CHAINS];
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) c[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (want_chains) {
#pragma unroll
      for (uint32_t g = 0; g < CHAINS; ++g) c[g] = chains[(size_t)g * n4 + (size_t)k * TILE_SLOTS + slot];  // layer 0 of chain g
    }
    float4 alb = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nrm = alb;
    if (inside && n_total != 0) {
      const size_t i = (size_t)y * L.grid.width + x;
      if (F & RENE_FEATURE_ALBEDO) alb = image[2 * n_px + i];
      if (F & RENE_FEATURE_NORMAL) nrm = image[n_px + i];
    }
    uint32_t ch = 0;
    auto emit = [&](float v) {  // the next channel of this thread's pixel
      const T e = to_element<T>(v);
      if (HWC) s_stage[threadIdx.x * C + ch] = e;
      else if (inside) dst[((size_t)ch * L.grid.height + y) * L.grid.width + x] = e;
      ++ch;
    };
    float mr = 0.0f, mg = 0.0f, mb = 0.0f;  // COLOR
    if (n_total != 0) {
      // S0 = ((C_0 + C_1) + ...) + C_7 exactly as rene_download resolves it: it starts from C_0, not from 0 -- 0 + (-0.0) is +0.0, and COLOR is
      // bit for bit rene_download_mean's, whose sum of eight -0.0 is -0.0
      float sr = c[0].x, sg = c[0].y, sb = c[0].z;
#pragma unroll
      for (uint32_t g = 1; g < CHAINS; ++g) {
        sr += c[g].x;
        sg += c[g].y;
        sb += c[g].z;
      }
      mr = sr / n_total_f;
      mg = sg / n_total_f;
      mb = sb / n_total_f;
    }
    if (F & RENE_FEATURE_COLOR) {
      emit(mr);
      emit(mg);
      emit(mb);
    }
    if (F & RENE_FEATURE_ALBEDO) {
      emit(n_total ? alb.x / n_total_f : 0.0f);
      emit(n_total ? alb.y / n_total_f : 0.0f);
      emit(n_total ? alb.z / n_total_f : 0.0f);
    }
    if (F & RENE_FEATURE_NORMAL) {
      emit(n_total ? nrm.x / n_total_f : 0.0f);
      emit(n_total ? nrm.y / n_total_f : 0.0f);
      emit(n_total ? nrm.z / n_total_f : 0.0f);
    }
    if (F & RENE_FEATURE_VARIANCE) {
      float v = 0.0f;
      if (kk >= 2u) {
        const float l = lum3(mr, mg, mb);
#pragma unroll
        for (uint32_t g = 0; g < CHAINS; ++g) {
          if (!cn[g]) continue;
          const float t = lum3(c[g].x / nf[g], c[g].y / nf[g], c[g].z / nf[g]) - l;
          v = v + share[g] * (t * t);
        }
        v = v / (float)(kk - 1u);
      }
      emit(v);
    }
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      if (!(F & (h ? RENE_FEATURE_HALF_B : RENE_FEATURE_HALF_A))) continue;
      float ar = 0.0f, ag = 0.0f, ab = 0.0f;
      if (n_half[h] != 0) {
        ar = ((c[h].x + c[h + 2].x) + c[h + 4].x) + c[h + 6].x;
        ag = ((c[h].y + c[h + 2].y) + c[h + 4].y) + c[h + 6].y;
        ab = ((c[h].z + c[h + 2].z) + c[h + 4].z) + c[h + 6].z;
        ar = ar / half_f[h];
        ag = ag / half_f[h];
        ab = ab / half_f[h];
      }
      emit(ar);
      emit(ag);
      emit(ab);
    }
    if (F & RENE_FEATURE_FRAMES) emit(n_total_f);
    if (HWC) {
      __syncthreads();
      // wave w copies rows w and w + 4 of the step: row_px * C consecutive elements each, consecutive lanes to consecutive elements
      const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, row_len = row_px * C;
#pragma unroll
      for (uint32_t r = wave; r < FEAT_STEP_ROWS; r += FEAT_WAVES) {
        const uint32_t yr = y0 + q * FEAT_STEP_ROWS + r;
        if (yr >= L.grid.height) continue;
        const T* src = s_stage + (size_t)r * RENE_TILE_SIZE * C;
        T* out = dst + ((size_t)yr * L.grid.width + x0) * C;
        for (uint32_t e = lane; e < row_len; e += 64u) out[e] = src[e];
      }
      __syncthreads();  // the stage is written again by the next step
    }
  }
}

hipError_t launch_features(const float* chains, const float* image, void* dst, int format, int layout, const FeatureLaunch& L, hipStream_t st) {
  const uint32_t n_owned = L.grid.n_slots / TILE_SLOTS;
  if (n_owned == 0) return hipSuccess;
  if (L.channels == 0 || L.channels > FEAT_MAX_CHANNELS) return hipErrorInvalidValue;
  const float4* c4 = reinterpret_cast<const float4*>(chains);
  const float4* i4 = reinterpret_cast<const float4*>(image);
  const dim3 grid(n_owned), block(FEAT_BLOCK);
  const bool hwc = layout == RENE_FEATURES_HWC;
  if (format == RENE_FEATURES_F16) {
    if (hwc) hipLaunchKernelGGL((features_kernel<_Float16, true>), grid, block, 0, st, c4, i4, static_cast<_Float16*>(dst), L);
    else hipLaunchKernelGGL((features_kernel<_Float16, false>), grid, block, 0, st, c4, i4, static_cast<_Float16*>(dst), L);
  } else {
    if (hwc) hipLaunchKernelGGL((features_kernel<float, true>), grid, block, 0, st, c4, i4, static_cast<float*>(dst), L);
    else hipLaunchKernelGGL((features_kernel<float, false>), grid, block, 0, st, c4, i4, static_cast<float*>(dst), L);
  }
  return hipGetLastError();
}

}  // namespace rene
