// kernels_denoise.hip -- the build-defined denoiser `atrous` (rene_denoise, include/rene_hip.h): an edge-avoiding a-trous wavelet filter
// (Dammertz et al. 2010; the spatial half of SVGF, Schied et al. 2017) guided by the first-hit normal and albedo layers and by the variance of
// the pixel's mean, which the eight frame chains (device_scene.h, CHAINS) give for nothing: eight independent sub-means per pixel.
//
//   prepare   one thread per owned pixel slot (chain_pass.h maps it to its pixel): reads the pixel's eight radiance records and the resolved guide layers, writes pixel-major records
//             rec[y][x] = {demodulated colour.rgb, variance of the mean of its luminance} and the constant guides g0 = {normal.xyz, albedo.r},
//             g1 = {albedo.g, albedo.b, 0, 0} (fp32: 16 + 32 bytes per pixel), and the unfiltered variance plane
//   pass      one launch per iteration i (step s = 2^i), one thread per pixel, 25 taps of three 16-byte loads each.  For small steps the
//             workgroup's 32 x 8 tile and a halo of 2 s pixels are staged in LDS (atrous_pass_kernel<S>, S > 0); the larger steps read their
//             taps through L2 (S == 0: consecutive lanes stay on consecutive records).  Both do the same arithmetic in the same order
//   finalize  remodulates and scales by the frame count: the unit of rene_download
//
// Nothing here writes the accumulation state: chains and image are read only.
#include <hip/hip_runtime.h>

#include "chain_pass.h"

namespace rene {

namespace {

constexpr int DN_TX = 32, DN_TY = 8;  // a workgroup's tile: 32 x 8 pixels, a wave = two rows of 32.  ds_read_b128 resolves bank conflicts inside
                                      // 16-lane groups that lie within one 32-lane half, and 32 consecutive lanes reading 32 consecutive 16-byte
                                      // records cover every bank once per group whatever the row's base: rows need no padding at this width
constexpr int DN_BLOCK = DN_TX * DN_TY;

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

}  // namespace

__global__ void __launch_bounds__(256) denoise_prepare_kernel(const float4* __restrict__ chains, const float4* __restrict__ image, float4* __restrict__ rec,
                                                              float4* __restrict__ guides, float* __restrict__ var_plane, DenoiseLaunch D) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // owned pixel slot (an unsharded context: tile = slot / 1024)
  if (i >= D.grid.n_slots) return;
  const uint32_t s = (uint32_t)i;
  const uint2 o = image_tile_origin(D.grid, s / TILE_SLOTS), d = slot_pixel(s % TILE_SLOTS);
  const uint32_t x = o.x + d.x, y = o.y + d.y;
  if (x >= D.grid.width || y >= D.grid.height) return;
  const size_t n4 = (size_t)3 * D.grid.n_slots, p = (size_t)y * D.grid.width + x, np = (size_t)D.grid.width * D.grid.height;
  float4 c[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) c[g] = chains[(size_t)g * n4 + i];  // layer 0 of chain g
  float sr = c[0].x, sg = c[0].y, sb = c[0].z;  // ((c0 + c1) + c2) + ... like resolve_chains_kernel
#pragma unroll
  for (uint32_t g = 1; g < CHAINS; ++g) {
    sr += c[g].x;
    sg += c[g].y;
    sb += c[g].z;
  }
  const float4 s1 = image[np + p], s2 = image[2 * np + p];
  const float nx = s1.x * D.inv_n, ny = s1.y * D.inv_n, nz = s1.z * D.inv_n;
  const float ar = s2.x * D.inv_n, ag = s2.y * D.inv_n, ab = s2.z * D.inv_n;
  const float ir = 1.0f / (ar + D.albedo_floor), ig = 1.0f / (ag + D.albedo_floor), ib = 1.0f / (ab + D.albedo_floor);
  const float dr = sr * D.inv_n * ir, dg = sg * D.inv_n * ig, db = sb * D.inv_n * ib;
  const float lm = lum3(dr, dg, db);
  float var = 0.0f;
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    if (D.chain_share[g] > 0.0f) {  // chains that have received frames
      const float t = lum3(c[g].x * D.chain_inv[g] * ir, c[g].y * D.chain_inv[g] * ig, c[g].z * D.chain_inv[g] * ib) - lm;
      var += D.chain_share[g] * (t * t);
    }
  }
  var *= D.inv_km1;
  rec[p] = make_float4(dr, dg, db, var);
  guides[2 * p] = make_float4(nx, ny, nz, ar);
  guides[2 * p + 1] = make_float4(ag, ab, 0.0f, 0.0f);
  var_plane[p] = var;
}

// S > 0: the tile and a halo of 2 S pixels staged in LDS, step S; S == 0: step D.step, every tap from global memory
template <int S>
__global__ void __launch_bounds__(DN_BLOCK) atrous_pass_kernel(const float4* __restrict__ rec, const float4* __restrict__ guides, float4* __restrict__ out, DenoiseLaunch D) {
  constexpr int HALO = 2 * S, LW = DN_TX + 2 * HALO, LH = DN_TY + 2 * HALO, LN = S ? LW * LH : 1;
  __shared__ float4 t_rec[LN], t_g0[LN], t_g1[LN];
  const int W = (int)D.grid.width, H = (int)D.grid.height;
  // Which tile this workgroup filters.  Workgroups are dealt round-robin over the chip's eight XCDs, each with an L2 of its own: with tiles in
  // launch order the eight neighbours of a tile sit behind eight different L2s and every one of them fetches the halo for itself (measured: a
  // step-8 pass read ten times the records' bytes through the L2s' memory side).  D.tile_columns > 0: XCD k (workgroups k, k + 8, ...) takes the
  // k-th eighth of the tiles in an order that walks super-columns of D.tile_columns tiles, row by row, so that the tiles in flight behind one L2
  // are neighbours.  Only the order changes: no pixel's arithmetic does.
  const uint32_t gx = (D.grid.width + DN_TX - 1) / DN_TX, gy = (D.grid.height + DN_TY - 1) / DN_TY;
  uint32_t bx, by;
  if (D.tile_columns) {
    const uint32_t tile = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);  // (the grid is a multiple of eight workgroups)
    if (tile >= gx * gy) return;
    const uint32_t cw = D.tile_columns, full = gx / cw, per = cw * gy, sc = tile / per;
    if (sc < full) {
      const uint32_t r = tile - sc * per;
      by = r / cw;
      bx = sc * cw + r % cw;
    } else {  // the last, narrower super-column
      const uint32_t wl = gx - full * cw, r = tile - full * per;
      by = r / wl;
      bx = full * cw + r % wl;
    }
  } else {
    if (blockIdx.x >= gx * gy) return;
    by = blockIdx.x / gx;
    bx = blockIdx.x - by * gx;
  }
  const int x0 = (int)bx * DN_TX, y0 = (int)by * DN_TY;
  const int tx = (int)threadIdx.x & (DN_TX - 1), ty = (int)threadIdx.x / DN_TX;
  const int x = x0 + tx, y = y0 + ty;
  if constexpr (S > 0) {
    for (int k = (int)threadIdx.x; k < LN; k += DN_BLOCK) {
      const int ly = k / LW, lx = k - ly * LW, gx = x0 - HALO + lx, gy = y0 - HALO + ly;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {  // (texels outside the image stay unwritten and are never read: their taps are skipped)
        const size_t q = (size_t)gy * W + gx;
        t_rec[k] = rec[q];
        t_g0[k] = guides[2 * q];
        t_g1[k] = guides[2 * q + 1];
      }
    }
    __syncthreads();
  }
  if (x >= W || y >= H) return;
  const int step = S ? S : (int)D.step;
  const int lc = (ty + HALO) * LW + tx + HALO;  // S: the pixel's place in the staged tile
  const size_t p = (size_t)y * W + x;
  Centre c;
  if (S) {
    c.rec = t_rec[lc];
    c.g0 = t_g0[lc];
    c.g1 = t_g1[lc];
  } else {
    c.rec = rec[p];
    c.g0 = guides[2 * p];
    c.g1 = guides[2 * p + 1];
  }
  c.lum = lum3(c.rec.x, c.rec.y, c.rec.z);
  {  // 3 x 3 filter (1 2 1) x (1 2 1) / 16 of the variance, taps outside the image skipped and the weights renormalised
    float gv = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const float w = (float)((2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx))) * 0.0625f;
        const float v = S ? t_rec[lc + dy * LW + dx].w : rec[(size_t)qy * W + qx].w;
        gv += w * v;
        gw += w;
      }
    }
    c.sd = D.sigma_l * sqrtf(fmaxf(gv / gw, 0.0f));
  }
  Acc a{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int iy = -2; iy <= 2; ++iy) {
    const int qy = y + iy * step;
    if (qy < 0 || qy >= H) continue;
#pragma unroll
    for (int ix = -2; ix <= 2; ++ix) {
      const int qx = x + ix * step;
      if (qx < 0 || qx >= W) continue;
      const float h = h5(ix) * h5(iy);
      if (S) {
        const int k = lc + iy * S * LW + ix * S;
        tap(c, D, h, t_rec[k], t_g0[k], t_g1[k], a);
      } else {
        const size_t q = (size_t)qy * W + qx;
        tap(c, D, h, rec[q], guides[2 * q], guides[2 * q + 1], a);
      }
    }
  }
  const float iw = 1.0f / a.w;  // the centre tap alone weighs 9 / 64
  out[p] = make_float4(a.r * iw, a.g * iw, a.b * iw, a.v * (iw * iw));
}

__global__ void __launch_bounds__(256) denoise_finalize_kernel(const float4* __restrict__ rec, const float4* __restrict__ guides, float4* __restrict__ out, DenoiseLaunch D) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)D.grid.width * D.grid.height) return;
  const float4 c = rec[p], g0 = guides[2 * p], g1 = guides[2 * p + 1];
  out[p] = make_float4(c.x * (g0.w + D.albedo_floor) * D.n_frames, c.y * (g1.x + D.albedo_floor) * D.n_frames, c.z * (g1.y + D.albedo_floor) * D.n_frames, 0.0f);
}

hipError_t launch_denoise_prepare(const float* chains, const float* image, float* rec, float* guides, float* var_plane, const DenoiseLaunch& D, hipStream_t st) {
  if (D.grid.n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3((D.grid.n_slots + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<const float4*>(chains),
                     reinterpret_cast<const float4*>(image), reinterpret_cast<float4*>(rec), reinterpret_cast<float4*>(guides), var_plane, D);
  return hipGetLastError();
}

// steps up to `stage_max` go through the LDS-staged kernel.  The default is RENE_DENOISE_STAGE_MAX (-DRENE_DENOISE_STAGE_MAX=0 builds a library that
// never stages: the A/B of DESIGN.md section 4c); the environment variable of the same name overrides it per call (rene_hip.cpp)
#ifndef RENE_DENOISE_STAGE_MAX
#define RENE_DENOISE_STAGE_MAX 4
#endif
int denoise_stage_max() { return RENE_DENOISE_STAGE_MAX; }

hipError_t launch_atrous_pass(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, int stage_max, hipStream_t st) {
  const uint32_t tiles = ((D.grid.width + DN_TX - 1) / DN_TX) * ((D.grid.height + DN_TY - 1) / DN_TY);  // (at most 2^21 at 16384 x 16384)
  const dim3 grid((tiles + 7u) & ~7u), block(DN_BLOCK);
  const float4* r = reinterpret_cast<const float4*>(rec);
  const float4* g = reinterpret_cast<const float4*>(guides);
  float4* o = reinterpret_cast<float4*>(out);
  const uint32_t s = D.step <= (uint32_t)(stage_max < 0 ? 0 : stage_max) ? D.step : 0u;
  if (s == 1) hipLaunchKernelGGL(atrous_pass_kernel<1>, grid, block, 0, st, r, g, o, D);
  else if (s == 2) hipLaunchKernelGGL(atrous_pass_kernel<2>, grid, block, 0, st, r, g, o, D);
  else if (s == 4) hipLaunchKernelGGL(atrous_pass_kernel<4>, grid, block, 0, st, r, g, o, D);
  else hipLaunchKernelGGL(atrous_pass_kernel<0>, grid, block, 0, st, r, g, o, D);
  return hipGetLastError();
}

hipError_t launch_denoise_finalize(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, hipStream_t st) {
  const size_t n = (size_t)D.grid.width * D.grid.height;
  hipLaunchKernelGGL(denoise_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(rec),
                     reinterpret_cast<const float4*>(guides), reinterpret_cast<float4*>(out), D);
  return hipGetLastError();
}

}  // namespace rene
