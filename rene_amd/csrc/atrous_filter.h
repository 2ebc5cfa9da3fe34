// atrous_filter.h -- what the kernels of the `atrous` denoiser (kernels_denoise.hip, which alone includes it) do not spell out themselves: the
// shapes of their workgroups, one tap of the 5 x 5 kernel, its weights, and the mark of a pixel that takes part in the filter.
#pragma once
#include <hip/hip_runtime.h>

#include "chain_pass.h"

namespace rene {

constexpr int DN_TX = 32, DN_TY = 8;  // a workgroup's tile: 32 x 8 pixels, a wave = two rows of 32.  ds_read_b128 resolves bank conflicts inside
                                      // 16-lane groups that lie within one 32-lane half, and 32 consecutive lanes reading 32 consecutive 16-byte
                                      // records cover every bank once per group whatever the row's base: rows need no padding at this width
constexpr int DN_BLOCK = DN_TX * DN_TY;
constexpr uint32_t DN_PREPARE_BLOCK = 256;  // prepare: a workgroup's consecutive slots lie inside one owned tile (TILE_SLOTS is a multiple of it)

// one tap of the 5 x 5 kernel: weight h * exp(-e) of the pixel (rq, a0, a1) seen from (rp, p0, p1)
struct Centre {
  float4 rec, g0, g1;
  float lum, sd;
};
struct Acc {
  float r, g, b, v, w;
};
__device__ __forceinline__ void tap(const Centre& c, const DenoiseLaunch& D, float h, const float4& rq, const float4& q0, const float4& q1, Acc& a) {
  const float nx = c.g0.x - q0.x, ny = c.g0.y - q0.y, nz = c.g0.z - q0.z;
  const float ar = c.g0.w - q0.w, ag = c.g1.x - q1.x, ab = c.g1.y - q1.y;
  const float lq = lum3(rq.x, rq.y, rq.z);
  const float e = (nx * nx + ny * ny + nz * nz) * D.inv_sigma_n2 + (ar * ar + ag * ag + ab * ab) * D.inv_sigma_a2 +
                  fabsf(c.lum - lq) / (c.sd + D.relative_floor * (fabsf(c.lum) + fabsf(lq)) + 1e-12f);
  const float w = h * __expf(-e);  // one v_exp_f32
  a.r += w * rq.x;
  a.g += w * rq.y;
  a.b += w * rq.z;
  a.v += w * w * rq.w;
  a.w += w;
}
__device__ __forceinline__ float h5(int k) { return k == 0 ? 0.375f : (k == 1 || k == -1) ? 0.25f : 0.0625f; }

// is the pixel whose second guide record is g1 part of the filter?  (denoise_prepare_kernel, TILES: .z)
__device__ __forceinline__ bool dn_valid(const float4& g1) { return g1.z != 0.0f; }

}  // namespace rene
